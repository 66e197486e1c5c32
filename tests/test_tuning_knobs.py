"""The DZO_TUNE_* environment variables: one list, held against the sources.  A knob exists only while somebody reads it -- a
test, bench.py, a tool that still answers a question -- or it is DZO_TUNE_POLL, the one operational escape hatch.  Every
variable is read through tune_int (csrc/dzo_common.h), and DESIGN.md lists the same set between two markers."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dzoptimization.jl_amd", "csrc")
BEGIN, END = "<!-- tuning-knobs:begin -->", "<!-- tuning-knobs:end -->"

# name -> (the unit that reads it, who sets it)
KNOBS = {
    "ADGD_FUSED": ("dzo_adgd.hip", "tests/test_gpu_bfgs.py"),
    "ADGD_PIPELINE": ("dzo_adgd.hip", "tests/test_gpu_bfgs.py"),
    "ADGD_PROLOGUE": ("dzo_adgd.hip", "tests/test_gpu_bfgs.py"),
    "BATCH_DEBUG": ("dzo_batch.hip", "tools/batch_phases.py"),
    "BATCH_RP2_WIDE_ABOVE": ("dzo_batch.hip", "tests/test_bfgs_twin.py"),
    "BFGS_COLS": ("dzo_bfgs.hip", "tests/test_gpu_bfgs_shapes.py"),
    "BFGS_DEV_ROUNDS": ("dzo_bfgs.hip", "tests/test_gpu_bfgs.py"),
    "BFGS_DEV_SEARCH": ("dzo_bfgs.hip", "tests/test_gpu_bfgs.py"),
    "BFGS_DUAL_SEARCH": ("dzo_bfgs.hip", "tests/test_gpu_bfgs.py"),
    "BFGS_PHI_FUSED": ("dzo_bfgs.hip", "tests/test_gpu_bfgs.py"),
    "BFGS_TRI_MIN_N": ("dzo_bfgs.hip", "tests/test_gpu_bfgs_shapes.py"),
    "FAST_DIV": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "FUSED_FINISH": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "FUSED_POST": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "FUSED_TRIAL": ("dzo_optcore.hip", "tests/test_gpu_lbfgs.py"),
    "GENERIC_POST": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "LSE_POINTS": ("dzo_lbfgs.hip", "bench.py"),
    "PAIRWISE_WAVE_MAX": ("dzo_pairwise.hip", "tools/bench_pairwise.py"),
    "PHI6_COLS": ("dzo_problems.hip", "tests/test_gpu_bfgs_steps.py"),
    "POINT_PRIO": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs_scale.py"),
    "POINT_RING": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "POINT_SETS": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs_scale.py"),
    "POLL": ("dzo_core.hip", "operational"),
    "SINGLE_PASS": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "SPECULATE": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs.py"),
    "SP_DEBUG": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs_scale.py"),
    "STREAM_MAJOR": ("dzo_lbfgs.hip", "tests/test_gpu_lbfgs_scale.py"),
    "TP_DEBUG": ("dzo_lbfgs.hip", "tools/wave_times.py"),
}

# folded into their defaults; the variants they selected are gone
FOLDED = ["STRIDE_SKEW", "BLOCKED", "INTERLEAVE", "LAZY_D", "GRAM_U", "COMBINE_U", "GRAM_BPC", "COMBINE_BPC", "FUSED_FINISH_MAX",
          "GRAM_VARIANT", "COMBINE_NTS", "SP_RETRY", "POINT_STAGE_ROWS", "POINT_PLAIN_MB", "POINT_LEFTOVER_EVEN", "GRAM_PEEL",
          "GRAM_FRESH_PLAIN", "GRAM_SKIP0", "COMBINE_FRESH_PLAIN", "ADGD_BPC", "ADGD_NT_STORES"]


def code_of(path):
    """The file without its // comments (as tests/test_lbfgs_plan.py strips them)."""
    return "\n".join(line.split("//")[0] for line in open(path).read().splitlines())


def csrc_code():
    return {name: code_of(os.path.join(CSRC, name)) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


def test_the_list_has_28_names_and_21_left():
    assert len(KNOBS) == 28 and len(FOLDED) == 21 and not set(KNOBS) & set(FOLDED)
    assert [name for name, (_, reader) in KNOBS.items() if reader == "operational"] == ["POLL"]


def test_the_sources_read_exactly_the_listed_knobs():
    code = csrc_code()
    found = {name for text in code.values() for name in re.findall(r"DZO_TUNE_([A-Z0-9_]+)", text)}
    assert found == set(KNOBS), (sorted(found - set(KNOBS)), sorted(set(KNOBS) - found))
    for name, (unit, _) in KNOBS.items():
        assert '"DZO_TUNE_%s"' % name in code[unit], (name, unit)


def test_every_knob_has_its_reader():
    for name, (_, reader) in KNOBS.items():
        if reader == "operational":
            continue
        assert reader == "bench.py" or reader.startswith(("tests/", "tools/")), (name, reader)
        assert re.search(r"DZO_TUNE_%s(?![A-Z0-9_])" % name, open(os.path.join(ROOT, reader)).read()), (name, reader)


def test_one_function_reads_the_environment():
    """getenv( occurs once in the code of csrc/: inside tune_int."""
    code = csrc_code()
    counts = {name: text.count("getenv(") for name, text in code.items() if "getenv(" in text}
    assert counts == {"dzo_common.h": 1}, counts
    common = code["dzo_common.h"]
    body = common[common.index("static inline int tune_int(const char *name, int dflt)"):]
    assert "getenv(" in body[:body.index("\n}\n")]


def test_design_lists_the_same_knobs():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.count(BEGIN) == 1 and design.count(END) == 1
    section = design[design.index(BEGIN) + len(BEGIN):design.index(END)]
    named = re.findall(r"DZO_TUNE_([A-Z0-9_]+)", section)
    assert sorted(named) == sorted(KNOBS), (sorted(set(named) ^ set(KNOBS)), len(named))


def test_no_folded_knob_is_named_anywhere():
    """Neither as DZO_TUNE_<name> nor as a bare quoted key (the plan driver's and the twin's spelling)."""
    patterns = [re.compile(r"""(?:DZO_TUNE_|["'])%s(?![A-Z0-9_])""" % name) for name in FOLDED]
    own = os.path.abspath(__file__)
    for top in ("dzoptimization.jl_amd", "tools", "tests"):
        for folder, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ("build", "__pycache__", "bin", "golden")]
            for name in files:
                path = os.path.join(folder, name)
                raw = open(path, "rb").read()
                if path == own or b"\0" in raw:                                   # (a built library is not a source)
                    continue
                text = raw.decode("utf-8", errors="replace")
                hits = [p.pattern for p in patterns if p.search(text)]
                assert not hits, (os.path.relpath(path, ROOT), hits)
