"""``dzo.PathwayGraph`` on hand-made graphs: connectivity, the minimax path and its tie rule, zero-weight edges, the attempt
limit, and the choice of a gap through an intermediate minimum.  Pure host code: no device, no library call."""
import inspect

from dzo_loader import dzo


def _graph(n_minima, saddles=(), max_attempts=2):
    g = dzo.PathwayGraph(max_attempts)
    for k in range(n_minima):
        assert g.add_minimum(-10.0 - k) == k
    for energy, i, j in saddles:
        g.add_saddle(energy, i, j)
    return g


def test_connectivity():
    g = _graph(5, [(-1.0, 0, 1), (-2.0, 1, 2), (-3.0, 3, 4)])
    assert g.n_minima == 5 and g.n_saddles == 3 and g.edges == [(0, 0, 1), (1, 1, 2), (3, 2, 4)]
    assert g.connected(0, 1) and g.connected(0, 2) and g.connected(2, 0) and g.connected(3, 4) and g.connected(2, 2)
    assert not g.connected(0, 3) and not g.connected(2, 4)
    assert g.best_path(0, 3) is None and g.best_path(2, 2) == [2]
    g.add_saddle(-0.5, 2, 3)
    assert g.connected(0, 4) and g.best_path(0, 4) == [0, 0, 1, 1, 2, 3, 3, 2, 4]


def test_best_path_minimises_the_highest_saddle():
    # 0 -1.0- 3 directly; 0 -2.0- 1 -3.0- 2 -2.5- 3 round about: lower at its highest point, so the longer way wins
    g = _graph(4, [(-1.0, 0, 3), (-2.0, 0, 1), (-3.0, 1, 2), (-2.5, 2, 3)])
    assert g.best_path(0, 3) == [0, 1, 1, 2, 2, 3, 3]
    assert g.best_path(3, 0) == [3, 3, 2, 2, 1, 1, 0]
    assert max(g.saddle_energies[s] for s in g.best_path(0, 3)[1::2]) == -2.0
    # two saddles between one pair of minima: the lower one is taken
    g = _graph(2, [(-1.0, 0, 1), (-4.0, 0, 1), (-2.0, 1, 0)])
    assert g.best_path(0, 1) == [0, 1, 1]


def test_best_path_breaks_ties_by_fewer_steps():
    # both ways peak at -2.0: one in two steps, one in three (its other saddles are lower)
    g = _graph(5, [(-2.0, 0, 1), (-5.0, 1, 2), (-6.0, 2, 4), (-2.0, 0, 3), (-2.0, 3, 4)])
    assert g.best_path(0, 4) == [0, 3, 3, 4, 4]
    # ... and the order of insertion does not decide it
    g = _graph(5, [(-2.0, 0, 3), (-2.0, 3, 4), (-2.0, 0, 1), (-5.0, 1, 2), (-6.0, 2, 4)])
    assert g.best_path(0, 4) == [0, 0, 3, 1, 4]


def test_best_path_takes_the_fewest_steps_when_the_peak_comes_late():
    """A way that is lower for a while but longer must not hide the shorter one once a later saddle sets the peak for both:
    0 -(-2)- 1 directly, 0 -(-5)- 3 -(-5)- 4 -(-5)- 1 round about, then 1 -(-2)- 2 for everyone."""
    g = _graph(5, [(-2.0, 0, 1), (-5.0, 0, 3), (-5.0, 3, 4), (-5.0, 4, 1), (-2.0, 1, 2)])
    assert g.best_path(0, 2) == [0, 0, 1, 4, 2]
    assert g.best_path(2, 0) == [2, 4, 1, 0, 0]
    assert g.best_path(0, 1) == [0, 1, 3, 2, 4, 3, 1]        # here the detour is lower at its highest point
    # the same with the peak in the middle: 0 -(-5)- 1 -(-1)- 2 -(-5)- 3, and long low detours on both sides
    g = _graph(8, [(-5.0, 0, 1), (-1.0, 1, 2), (-5.0, 2, 3), (-6.0, 0, 4), (-6.0, 4, 5), (-6.0, 5, 1), (-6.0, 2, 6), (-6.0, 6, 7), (-6.0, 7, 3)])
    assert g.best_path(0, 3) == [0, 0, 1, 1, 2, 2, 3]


def _with_distances(g, table):
    for (i, j), d in table.items():
        g.set_distance(i, j, d)
    return g


def test_next_attempts_takes_the_direct_gap_when_it_is_the_shortest():
    g = _with_distances(_graph(3), {(0, 1): 1.0, (1, 2): 1.0, (0, 2): 1.2})
    assert g.next_attempts(0, 2) == [(0, 2)]                 # 1.44 < 1 + 1
    assert g.distance(2, 0) == 1.2 and g.distance(1, 1) == 0.0 and g.distance(0, 1) == g.distance(1, 0)


def test_next_attempts_goes_through_an_intermediate_minimum_when_two_short_hops_beat_one_long_one():
    g = _with_distances(_graph(3), {(0, 1): 1.0, (1, 2): 1.0, (0, 2): 1.9})
    assert g.next_attempts(0, 2) == [(0, 1), (1, 2)]         # 1 + 1 < 3.61: d^2 favours the short hops, d would not (2 > 1.9)
    assert g.next_attempts(2, 0) == [(2, 1), (1, 0)]


def test_zero_weight_edges_are_crossed_for_free_and_not_returned():
    # 0 and 1 are joined already, 1 -> 3 is short: the way 0 => 1 -> 3 costs 0.25 against 1.0 directly
    g = _with_distances(_graph(4, [(-1.0, 0, 1)]), {(0, 1): 5.0, (0, 2): 3.0, (0, 3): 1.0, (1, 2): 3.0, (1, 3): 0.5, (2, 3): 3.0})
    assert g.next_attempts(0, 3) == [(1, 3)]
    g.add_saddle(-2.0, 1, 3)
    assert g.connected(0, 3) and g.next_attempts(0, 3) == []  # connected: the path is free, nothing is left to try
    # a joined pair costs nothing whatever its distance, also without a cached one
    g = _graph(3, [(-1.0, 0, 1)])
    g.set_distance(1, 2, 2.0)
    assert g.next_attempts(0, 2) == [(1, 2)]


def test_the_attempt_limit_turns_an_edge_infinite():
    g = _with_distances(_graph(3, max_attempts=2), {(0, 1): 1.0, (1, 2): 1.0, (0, 2): 1.2})
    assert g.next_attempts(0, 2) == [(0, 2)]
    g.note_attempt(0, 2)
    assert g.attempts(2, 0) == 1 and g.next_attempts(0, 2) == [(0, 2)]
    g.note_attempt(2, 0)                                     # the pair is the same in either direction
    assert g.attempts(0, 2) == 2 and g.next_attempts(0, 2) == [(0, 1), (1, 2)]
    for _ in range(2):
        g.note_attempt(0, 1)
    assert g.next_attempts(0, 2) == []                       # every way across is used up
    assert g.next_attempts(1, 2) == [(1, 2)]
    # a pair without a cached distance is never proposed
    g = _graph(2)
    assert g.next_attempts(0, 1) == []
    # a joined pair stays free however often it was tried
    g = _with_distances(_graph(3, [(-1.0, 0, 1)], max_attempts=1), {(0, 1): 1.0, (1, 2): 1.0, (0, 2): 9.0})
    g.note_attempt(0, 1)
    assert g.next_attempts(0, 2) == [(1, 2)]


def test_public_surface():
    for name in ("PathwayGraph", "PathwayConnections", "BandCandidates", "band_candidates", "connect_pathways"):
        assert name in dzo.__all__, name
    sig = inspect.signature(dzo.connect_pathways).parameters
    assert list(sig)[:4] == ["a", "b", "n_particles", "n_images"]
    for name in ("tol", "displacement"):
        assert sig[name].default is inspect.Parameter.empty and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["band_iterations"].default == 600 and sig["max_cycles"].default == 10 and sig["max_attempts"].default == 2
    assert sig["verify_index"].default is True
    for name in ("band_options", "align", "refine_options", "radial"):
        assert name in sig, name
    assert "NOT checked" in dzo.connect_pathways.__doc__ and "connect_saddles" in dzo.connect_pathways.__doc__
    assert list(inspect.signature(dzo.band_candidates).parameters)[:4] == ["band", "n_particles", "n_images", "energies"]
    assert inspect.signature(dzo.band_candidates).parameters["energies"].default is None
