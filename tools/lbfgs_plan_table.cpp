// lbfgs_plan_table.cpp -- stand-alone driver of csrc/dzo_lbfgs_plan.h (no GPU, no HIP):
//
//   lbfgs_plan_table            prints the decision table of DESIGN.md ("What runs": layout, arrangement, step path, kernel)
//   lbfgs_plan_table FILE       answers the queries of FILE, one per line, with the fields of the plan (tests/test_lbfgs_plan.py
//                               compares them with tests/lbfgs_plan_twin.py)
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined tools/lbfgs_plan_table.cpp -o lbfgs_plan_table
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../dzoptimization.jl_amd/csrc/dzo_lbfgs_plan.h"

using namespace dzo;

// ---------------------------------------------------------------------------- queries
// the knobs by the names of their DZO_TUNE_* variables
static bool set_knob(LbfgsKnobs &k, const char *name, int v) {
    struct { const char *name; int *p; } t[] = {
        {"SINGLE_PASS", &k.single_pass}, {"POINT_RING", &k.point_ring}, {"LSE_POINTS", &k.lse_points}, {"POINT_SETS", &k.point_sets},
        {"FUSED_FINISH", &k.fused_finish}, {"SPECULATE", &k.speculate}, {"FUSED_POST", &k.fused_post},
    };
    if (!strcmp(name, "STREAM_MAJOR")) { k.stream_major_set = true; k.stream_major = v; return true; }
    for (auto &e : t) if (!strcmp(name, e.name)) { *e.p = v; return true; }
    return false;
}

static int answer(FILE *in) {
    char line[512];
    while (fgets(line, sizeof line, in)) {
        char tag = 0;
        int used = 0;
        if (sscanf(line, " %c%n", &tag, &used) != 1) continue;
        const char *rest = line + used;
        if (tag == 'L') {
            // L n dtype m kind l2 bg cons x_al g_al c_al cus knob value
            long long n; int dtype, m, kind, bg, cons, xa, ga, ca, cus, kv; double l2; char kname[64];
            if (sscanf(rest, "%lld %d %d %d %lf %d %d %d %d %d %d %63s %d", &n, &dtype, &m, &kind, &l2, &bg, &cons, &xa, &ga, &ca, &cus, kname, &kv) != 13) return 2;
            LbfgsStart st;
            st.kind = kind; st.dec.l2 = l2; st.dec.bg_on = bg != 0; st.dec.cons_on = cons != 0;
            st.x_al16 = xa != 0; st.g_al16 = ga != 0; st.c_al16 = ca != 0;
            LbfgsKnobs kn;
            if (strcmp(kname, "-") && !set_knob(kn, kname, kv)) return 3;
            const LbfgsLayout L = lbfgs_plan_layout(n, dtype, m, st, kn, cus);
            printf("L %lld %d %d %d %d %lld %lld %lld %zu %lld %zu %zu %zu %zu %d %d %zu", (long long)L.stride, (int)L.blocked, (int)L.points,
                   L.ring_obj, L.nslots, (long long)L.ring_rows, (long long)L.tile_stride, (long long)L.rowbytes, L.ring_bytes,
                   (long long)L.pair_stride, L.slab_bytes, L.lin_bytes, L.d_bytes, L.d_offset, L.gram_grid, L.point_sets, L.scal.total);
            for (int i = 0; i < kScalCount; ++i) printf(" %zu", L.scal.off[i]);
            printf("\n");
        } else if (tag == 'V') {
            // V m dtype point_sets decorated obj first
            int m, dtype, sets, dec, obj, first;
            if (sscanf(rest, "%d %d %d %d %d %d", &m, &dtype, &sets, &dec, &obj, &first) != 6) return 2;
            const bool one = point_one_set(m, dtype, sets);
            const PassVariant v = point_pass_variant(m, dtype, one, dec != 0, obj, first != 0);
            printf("V %d %d %d %d %d %d %d %d\n", (int)one, v.K, v.SETS, (int)v.DEC, v.OBJ, (int)v.FIRST, pair_pass_k(m), lse_dots_k(m, dtype));
        } else if (tag == 'P') {
            // P n dtype m k point_sets regrad stage_rows prio plain_mb | rows resident gram_grid
            long long n, mb, rows, res; int dtype, m, k, sets, regrad, sr, prio, gg;
            if (sscanf(rest, "%lld %d %d %d %d %d %d %d %lld %lld %lld %d", &n, &dtype, &m, &k, &sets, &regrad, &sr, &prio, &mb, &rows, &res, &gg) != 12) return 2;
            const PointLaunch p = point_pass_launch(n, dtype, m, k, sets, regrad != 0, sr, prio, mb);
            printf("P %d %d %d %d %zu %d %d %d %zu %d %d\n", (int)p.one_set, p.stage_tiles, p.stage_max, p.stage_rows, p.stage_bytes, p.nt_tiles, p.prio,
                   point_stage_small_rows(p.stage_tiles), point_stage_bytes(point_stage_small_rows(p.stage_tiles), p.stage_tiles),
                   pass_grid(rows, res, gg, kPointPassGridCap), pass_grid(rows, res, gg, kPairPassGridCap));
        } else if (tag == 'S') {
            // S points single_pass blocked mode line_search descent sd speculate fused_post callbacks box has_problem iter n k m dtype
            //   ring_obj ring_decorated obj_agrees dec_agrees lambda_agrees lse_c_agrees spec_scalars d_al16
            long long iter, n; int v[23];
            if (sscanf(rest, "%d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5],
                       &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &iter, &n, &v[12], &v[13], &v[14], &v[15], &v[16], &v[17], &v[18], &v[19], &v[20],
                       &v[21], &v[22]) != 25) return 2;
            LbfgsStepFacts f;
            f.points = v[0]; f.single_pass = v[1]; f.blocked = v[2]; f.mode = v[3]; f.line_search = v[4]; f.descent_check = v[5];
            f.sd_fallback = v[6]; f.speculate = v[7]; f.fused_post = v[8]; f.callbacks = v[9]; f.box_on = v[10]; f.has_problem = v[11];
            f.iteration_count = iter; f.n = n; f.k = v[12]; f.m = v[13]; f.dtype = v[14]; f.ring_obj = v[15]; f.ring_decorated = v[16];
            f.obj_agrees = v[17]; f.dec_agrees = v[18]; f.lambda_agrees = v[19]; f.lse_c_agrees = v[20]; f.spec_scalars = v[21]; f.d_al16 = v[22];
            printf("S %d %d\n", (int)points_plan_ok(f), (int)(single_pass_plan_ok(f) && f.d_al16));
        } else if (tag == 'C') {
            printf("C %d %d %d %d %d %d %d %d %d %d %d\n", kPlanWaves, kPlanMaxHistory, kPlanMaxPartialBlocks, kGramValues, kRowOwn, kRowLead,
                   kTileBytes, kPairMaxK, kFusedMaxK, point_max_k(DZO_F64), point_max_k(DZO_F32));
        } else {
            return 2;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------- the table
struct Scenario {
    const char *objective, *decorators, *options, *shape;
    int kind; bool decorated, callbacks, plain_options, x_al, c_al;
    long long n;
    const char *pinned;                         // the case of tests/test_gpu_lbfgs_plan.py; "create": its second test; "cpu": tests/test_lbfgs_plan.py only
};

// the pytest id that pins ring, tiles and step of a row (the kernel column: test_kernel_variants_..., no getter reports a variant)
static std::string pinned_by(const Scenario &s, int dtype) {
    const std::string dt = dtype == DZO_F64 ? "float64" : "float32", p = s.pinned;
    if (p == "cpu") return "test_layout_matches_the_twin_over_the_whole_range";
    if (p == "create") return "test_create_without_a_problem_and_with_callbacks_is_never_blocked[" + dt + "]";
    return "test_handles_decide_what_the_twin_predicts[" + dt + "-" + p + "]";
}

static std::string describe(const Scenario &s, int dtype, int m) {
    LbfgsStart st;
    if (!s.callbacks) {
        st.kind = s.kind; if (s.decorated) st.dec.l2 = 0.5;
        st.x_al16 = s.x_al; st.g_al16 = true; st.c_al16 = s.c_al;
    }
    const LbfgsKnobs kn;
    const LbfgsLayout L = lbfgs_plan_layout(s.n, dtype, m, st, kn, 256);
    char buf[256];
    const char *tiles = !L.blocked ? "-" : (L.tile_stride == kTileBytes ? "tile-major" : "stream-major");
    // a step in the steady state (k = m pairs, scalars from the previous pass)
    LbfgsStepFacts f;
    f.points = L.points; f.single_pass = true; f.blocked = L.blocked; f.line_search = s.plain_options ? 0 : 1;
    f.callbacks = s.callbacks; f.has_problem = !s.callbacks; f.iteration_count = m; f.n = s.n; f.k = m; f.m = m; f.dtype = dtype;
    f.ring_obj = L.ring_obj; f.ring_decorated = st.dec.any(); f.obj_agrees = f.dec_agrees = f.lambda_agrees = f.lse_c_agrees = true;
    f.spec_scalars = true; f.d_al16 = true;
    const int64_t vecn = 16 / plan_dtype_size(dtype);
    if (points_plan_ok(f)) {
        if (L.ring_obj == 2) {
            snprintf(buf, sizeof buf, "points | %s | point pass (LSE) | `lse_trial` + `lse_dots<K=%d>`", tiles, lse_dots_k(m, dtype));
        } else {
            const PassVariant v = point_pass_variant(m, dtype, point_one_set(m, dtype, L.point_sets), st.dec.any(), L.ring_obj, false);
            snprintf(buf, sizeof buf, "points | %s | point pass | `<K=%d, SETS=%d, DEC=%d, OBJ=%d>`", tiles, v.K, v.SETS, (int)v.DEC, v.OBJ);
        }
        return buf;
    }
    if (L.points) {
        // an option the passes do not serve: the ring becomes a pair ring in place; a ragged n continues on the slabs
        const bool ragged = s.n % vecn != 0;
        snprintf(buf, sizeof buf, "points, then %s | %s | two-pass (Gram + combine) | -", ragged ? "slabs" : "pairs", ragged ? "-" : tiles);
        return buf;
    }
    snprintf(buf, sizeof buf, "%s | %s | two-pass (Gram + combine) | -", L.blocked ? "pairs" : "slabs", tiles);
    return buf;
}

static void table() {
    const long long N = 1000000;           // (small enough that a stream-major ring fits 32-bit byte offsets for every m)
    const Scenario rows[] = {
        {"Rosenbrock chain", "none", "plain", "n >= 4 vec, ragged too", DZO_PROBLEM_ROSENBROCK_CHAIN, false, false, true, true, true, N + 1, "rosen"},
        {"Rosenbrock chain", "L2 / box", "plain", "n >= 4 vec, ragged too", DZO_PROBLEM_ROSENBROCK_CHAIN, true, false, true, true, true, N, "rosen-dec"},
        {"Rosenbrock chain", "none", "Wolfe / safeguards / CHAIN", "n % vec = 0", DZO_PROBLEM_ROSENBROCK_CHAIN, false, false, false, true, true, N, "rosen"},
        {"Rosenbrock chain", "none", "Wolfe / safeguards / CHAIN", "ragged n", DZO_PROBLEM_ROSENBROCK_CHAIN, false, false, false, true, true, N + 1, "rosen"},
        {"Rosenbrock chain", "none", "plain", "n < 4 vec", DZO_PROBLEM_ROSENBROCK_CHAIN, false, false, true, true, true, 7, "rosen"},
        {"Rosenbrock chain", "none", "plain", "x or g off 16 B", DZO_PROBLEM_ROSENBROCK_CHAIN, false, false, true, false, true, N, "cpu"},
        {"quadratic chain", "none", "plain", "n >= 4 vec, ragged too", DZO_PROBLEM_QUADRATIC_CHAIN, false, false, true, true, true, N, "quad"},
        {"quadratic chain", "L2 / box", "plain", "any", DZO_PROBLEM_QUADRATIC_CHAIN, true, false, true, true, true, N, "quad-dec"},
        {"log-sum-exp", "none", "plain", "c on 16 B", DZO_PROBLEM_LSE, false, false, true, true, true, N, "lse"},
        {"log-sum-exp", "none", "plain", "c off 16 B", DZO_PROBLEM_LSE, false, false, true, true, false, N, "lse-c-off"},
        {"log-sum-exp", "L2 / box", "plain", "any", DZO_PROBLEM_LSE, true, false, true, true, true, N, "lse-dec"},
        {"dense quadratic", "any", "any", "any", DZO_PROBLEM_QUADRATIC, false, false, true, true, true, 4096, "cpu"},
        {"callbacks / `dzo_lbfgs_create`", "any", "any", "any", -1, false, true, true, true, true, N, "create"},
    };
    printf("| objective | decorators | options | shape | dtype | m | ring | tiles | step | kernel | ring, tiles and step pinned by |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|---|\n");
    for (const Scenario &s : rows) {
        for (int dtype : {DZO_F64, DZO_F32}) {
            const int top = 26;                 // (above point_max_k nothing changes up to kMaxHistory)
            int from = 1;
            std::string cur = describe(s, dtype, 1);
            for (int m = 2; m <= top + 1; ++m) {
                const std::string next = m <= top ? describe(s, dtype, m) : std::string();
                if (next == cur) continue;
                char range[32];
                if (m - 1 == top && from == 1) snprintf(range, sizeof range, "all");
                else if (m - 1 == top) snprintf(range, sizeof range, "%d+", from);
                else if (from == m - 1) snprintf(range, sizeof range, "%d", from);
                else snprintf(range, sizeof range, "%d-%d", from, m - 1);
                printf("| %s | %s | %s | %s | %s | %s | %s | %s |\n", s.objective, s.decorators, s.options, s.shape, dtype == DZO_F64 ? "fp64" : "fp32",
                       range, cur.c_str(), pinned_by(s, dtype).c_str());
                from = m; cur = next;
            }
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { table(); return 0; }
    FILE *in = fopen(argv[1], "r");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    const int rc = answer(in);
    fclose(in);
    if (rc) fprintf(stderr, "bad query (%d)\n", rc);
    return rc;
}
