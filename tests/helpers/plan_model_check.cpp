// plan_model_check.cpp -- csrc/sm_plan_model.h on the CPU, against the stand-in device of plan_cases.h.
//
//   plan_model_check dump      the cases of plan_cases.h, planned: the text tests/golden/plan_model_parent.json.gz holds
//   plan_model_check sweep     20 000 further seeded shapes: what every consumer of a geometry relies on
//   plan_model_check stats     how many of the match cases reach each branch of the planner
//   plan_model_check time      10^5 calls of each cost planner, five repetitions: ns per call
//   plan_model_check case K N  the inputs of case N of list K (0 match, 1 cost)
//   plan_model_check strips    the ghost-border strip kernels that some cost launch reaches, one name a line
//
// g++ -std=c++17 -Wall -Wextra; tests/test_plan_model_cpu.py builds and runs it.
#include <stdlib.h>

#include <chrono>

#include "plan_cases.h"
#include "plan_dump.h"

static int occupancy(void *, const KernelKey &k, int threads, int lds_bytes) { return standin_occupancy(k, threads, lds_bytes); }

static int plan_match(const PlanCase &c, MatchGeom *g, char (&describe)[512])
{
    const PlanDevice dev = {c.cus, occupancy, nullptr};
    return sm_plan_match(c.s, dev, g, describe, sizeof describe);
}

typedef CostKernelKey (*cost_planner)(const PlanShape &, int, bool, SadGeom *);
static const cost_planner COST_PLANNERS[3] = {sm_plan_sad_pc, sm_plan_sad_qs, sm_plan_ssd_mfma};
static const char *const COST_NAMES[3] = {"sad_pc", "sad_qs", "ssd_mfma"};

static int dump()
{
    printf("{");
    plan_dump_names(stdout);
    printf("\"match\":[\n");
    int i = 0;
    for (const PlanCase &c : plan_match_cases()) {
        MatchGeom g;
        char describe[512];
        const int kernel = plan_match(c, &g, describe);
        if (i++) printf(",\n");
        plan_dump_match(stdout, kernel, describe, g);
    }
    printf("\n],\n\"cost\":[\n");
    i = 0;
    for (const PlanCase &c : plan_cost_cases()) {
        printf(i++ ? ",\n[" : "[");
        for (int k = 0; k < 3; k++) {
            SadGeom q;
            memset(&q, 0xAA, sizeof q);
            plan_dump_cost(stdout, COST_PLANNERS[k](c.s, c.pairs, c.aligned4 != 0, &q).family, q);
            if (k < 2) printf(",");
        }
        printf("]");
    }
    printf("\n]}\n");
    return 0;
}

static void print_case(const PlanCase &c)
{
    const sm_plan_options &o = c.s.opt;
    printf("%dx%d D=%d square_width=%d border=%d max_pairs=%d cus=%d pairs=%d aligned4=%d kernel_family=%d tile_h=%d "
           "shifts_per_lane=%d workgroup_waves=%d no_two_wave_cap=%d lane_merge=%d no_four_shift_lanes=%d cost_kernel=%d "
           "cost_tile_h=%d cost_workgroup_waves=%d\n", c.s.w, c.s.h, c.s.D, c.s.square_width, c.s.border, c.s.max_pairs,
           c.cus, c.pairs, c.aligned4, o.kernel_family, o.tile_h, o.shifts_per_lane, o.workgroup_waves, o.no_two_wave_cap,
           o.lane_merge, o.no_four_shift_lanes, o.cost_kernel, o.cost_tile_h, o.cost_workgroup_waves);
}

// the LDS a bit-sliced geometry needs, without the pad that spreads a one-round grid
static int bs_lds_needed(const PlanCase &c, const MatchGeom &g)
{
    const PlanDevice dev = {c.cus, occupancy, nullptr};
    const MatchPlanner p = {c.s, dev, SM_KERNEL_BS, true, c.s.border == SM_GHOST, MatchGeom()};
    return MatchLds(p, g, g.plw + g.prw).bytes(g.tile_h);
}

static int stats()
{
    int bs = 0, tiled = 0, generic = 0, multi = 0, cap2 = 0, pad = 0, duo = 0, xmerge = 0, ds[3] = {0, 0, 0};
    for (const PlanCase &c : plan_match_cases()) {
        MatchGeom g;
        char describe[512];
        const int kernel = plan_match(c, &g, describe);
        if (kernel == SM_KERNEL_GENERIC) { generic++; continue; }
        const KernelKey k = sm_match_kernel_key(kernel, g, c.s.border == SM_GHOST);
        const long long tiles = (long long)g.tiles_x * g.tiles_y * c.s.max_pairs;
        multi += tiles > (long long)c.cus * std::max(1, standin_occupancy(k, g.threads, g.lds_bytes));
        if (kernel != SM_KERNEL_BS) { tiled++; continue; }
        bs++;
        cap2 += g.cap2; duo += g.duo; xmerge += g.xmerge;
        ds[g.ds == 16 ? 0 : g.ds == 8 ? 1 : 2]++;
        pad += g.lds_bytes != bs_lds_needed(c, g);
    }
    printf("bit_sliced=%d tiled=%d generic=%d multi_round=%d two_wave_variant=%d lds_pad=%d two_wave_workgroups=%d "
           "lane_merge_lds=%d ds16=%d ds8=%d ds4=%d\n", bs, tiled, generic, multi, cap2, pad, duo, xmerge, ds[0], ds[1], ds[2]);
    return 0;
}

// ---------------------------------------------------------------------------
// the property sweep
// ---------------------------------------------------------------------------

static int failures = 0;
#define EXPECT(cond)                                                                                                  \
    do {                                                                                                              \
        if (!(cond) && failures++ < 20) { printf("FAILED %s (line %d): ", #cond, __LINE__); print_case(c); }          \
    } while (0)

static void check_match(const PlanCase &c)
{
    MatchGeom g;
    char describe[512];
    const int kernel = plan_match(c, &g, describe);
    const sm_plan_options &o = c.s.opt;
    EXPECT(strlen(describe) > 0 && strlen(describe) < sizeof describe - 1);
    EXPECT(g.w == c.s.w && g.h == c.s.h && g.D == c.s.D && g.n == 2 * g.half + 1 && g.half == c.s.square_width / 2);
    EXPECT(g.ext_image_words == (long long)g.ext_words * g.ext_rows);
    EXPECT(g.edge_words_l <= g.ext_words && g.edge_words_r <= g.ext_words && g.edge_words_l <= g.edge_words_r);
    EXPECT(g.pad_l % 32 == 0 && g.pad_l >= g.half);
    EXPECT(o.kernel_family != 1 || kernel != SM_KERNEL_BS);
    if (kernel == SM_KERNEL_GENERIC) {
        EXPECT(g.D > 1024 || g.n > 25);
        EXPECT(g.ext_rows == g.h + 2 * g.half && 32 * g.ext_words >= g.pad_l + g.w + g.half + g.D + 32);
        return;
    }
    const bool bs = kernel == SM_KERNEL_BS;
    const int rows_per_wg = g.duo ? 2 : 1;
    EXPECT(g.lds_bytes > 0 && g.lds_bytes <= 64 * 1024);
    EXPECT(g.tile_h >= 1 && g.tile_h <= g.h);
    EXPECT((long long)g.tiles_x * g.tw >= g.w && (long long)(g.tiles_x - 1) * g.tw < g.w);
    EXPECT((long long)g.tiles_y * rows_per_wg * g.tile_h >= g.h && (long long)(g.tiles_y - 1) * rows_per_wg * g.tile_h < g.h);
    EXPECT(g.nsr == rows_per_wg * g.tile_h + g.n - 1);
    EXPECT(g.ext_words >= (g.tiles_x - 1) * g.tw / 32 + g.prw && g.ext_rows >= g.tiles_y * rows_per_wg * g.tile_h + g.n - 1);
    EXPECT(g.nl >= 1 && (g.nl & (g.nl - 1)) == 0 && g.nl == 1 << g.log2nl && g.nl * g.ds >= g.D && g.nl <= 64);
    EXPECT(g.nl == 1 || (g.nl / 2) * g.ds < g.D);
    EXPECT(bs ? (g.threads == 64 || g.threads == 128) && g.threads == (g.duo ? 128 : 64) && g.runs * g.nl == 64
              : g.threads <= 256 && g.threads == g.runs * g.nl && g.ds == SM_DSET && !g.duo && !g.cap2 && !g.xmerge);
    EXPECT(g.tw == (bs ? 32 : SM_P) * g.runs);
    EXPECT(g.vec_ok == (g.w % 4 == 0));
    if (!bs) { EXPECT(g.lds_bytes == g.nsr * (g.plw + g.prw) * 3 * 4); return; }
    EXPECT(sm_kernel_built(sm_match_kernel_key(kernel, g, c.s.border == SM_GHOST)));
    EXPECT(g.nl <= 32 && !(g.duo && g.cap2));
    EXPECT(g.lds_bytes >= bs_lds_needed(c, g));
    EXPECT(4 * g.nsr * (g.plw + g.prw) <= g.lds_bytes);
    if (g.xmerge) {
        EXPECT(g.log2nl >= 2 && g.xm_words > 0 && g.xm_off >= g.nsr * (g.plw + g.prw));
        EXPECT(4 * (g.xm_off + g.xm_words) <= g.lds_bytes && (!g.duo || g.xm_off - g.xm_words >= g.nsr * (g.plw + g.prw)));
    } else {
        EXPECT(g.xm_words == 0);
    }
    // an explicit option is honoured, or clamped as include/stereo_hip.h and the planner document
    int l2;
    if (o.tile_h > 0) EXPECT(g.tile_h <= std::min(o.tile_h, g.h) && (g.tile_h == std::min(o.tile_h, g.h) ||
                             MatchLds(MatchPlanner{c.s, PlanDevice{c.cus, occupancy, nullptr}, kernel, true, c.s.border == SM_GHOST,
                                                   MatchGeom()}, g, g.plw + g.prw).bytes(g.tile_h + 1) > 64 * 1024));
    if ((o.shifts_per_lane == 4 || o.shifts_per_lane == 8 || o.shifts_per_lane == 16) &&
        sm_bs_built(g.n, o.shifts_per_lane, false, false) && sm_lanes_for(g.D, o.shifts_per_lane, &l2) <= 32)
        EXPECT(g.ds == o.shifts_per_lane);
    if (o.no_four_shift_lanes && o.shifts_per_lane != 4) EXPECT(g.ds != 4);
    if (o.workgroup_waves == 1) EXPECT(!g.duo);
    if (o.workgroup_waves == 2) EXPECT(g.duo == (int)sm_bs_built(g.n, g.ds, false, true));
    if (o.no_two_wave_cap) EXPECT(!g.cap2);
    if (o.lane_merge == 1) EXPECT(!g.xmerge);
    if (o.lane_merge == 2) EXPECT(g.xmerge == (g.log2nl >= 2));
}

static void check_cost(const PlanCase &c)
{
    const int n = 2 * (c.s.square_width / 2) + 1;
    for (int k = 0; k < 3; k++) {
        SadGeom g;
        memset(&g, 0xAA, sizeof g);
        const CostKernelKey key = COST_PLANNERS[k](c.s, c.pairs, c.aligned4 != 0, &g);
        if (c.s.opt.cost_kernel == 1) EXPECT(key.family == SM_COST_KERNEL_NONE);
        if (key.family == SM_COST_KERNEL_NONE) continue;
        EXPECT(key.family == k + 1 && key.n == n);
        EXPECT(g.w == c.s.w && g.h == c.s.h && g.D == c.s.D && g.ghost == (c.s.border == SM_GHOST));
        EXPECT(g.waves == 1 || g.waves == 2 || g.waves == 4);
        EXPECT(64 * g.waves <= 256);
        // (80 KiB for the four-wave SAD shape only: sm_cost_wta raises that kernel's limit)
        EXPECT(g.lds_bytes > 0 && g.lds_bytes <= (k == 0 && g.waves == 4 ? 80 : 64) * 1024);
        EXPECT(g.tile_h >= 1 && g.tile_h <= g.h && g.nsr == g.tile_h + n - 1);
        EXPECT((long long)g.tiles_x * g.tw >= g.w && (long long)(g.tiles_x - 1) * g.tw < g.w);
        EXPECT((long long)g.tiles_y * g.tile_h >= g.h && (long long)(g.tiles_y - 1) * g.tile_h < g.h);
        EXPECT(g.nl >= 1 && (g.nl & (g.nl - 1)) == 0 && g.nl == 1 << g.log2nl && g.nl <= 16);
        EXPECT(g.lrow % 8 == 0 && g.rrow % 8 == 0 && g.padl % 4 == 0 && g.padl >= c.s.square_width / 2 + 3);
        EXPECT(g.nsr * (g.lrow + g.rrow) + 4 * g.tbl_pad <= g.lds_bytes);
        EXPECT(g.tbl_pad >= 0 && g.tbl_pad < 4 && (k == 2 || g.tbl_pad == 0));
        if (k < 2) {
            EXPECT(g.nql == key.nql && g.px == key.px && 4 * g.nl * g.nql >= g.D + 3 && g.tw == 4 * g.px * (16 / g.nl) * g.waves);
            EXPECT(g.q_tail >= 0 && g.q_last >= 0 && g.q_last <= g.nql - 1);
        } else {
            EXPECT(key.nb >= 1 && key.nb <= 9 && 32 * key.nb >= g.D + 31 && g.tw == 32 * g.waves);
            EXPECT((g.nsr * ((g.lrow + g.rrow) / 4) + g.tbl_pad) % 4 == 0);
        }
        if (g.fast_stage) {
            // the staging reach: 4 dwords a lane
            EXPECT(g.lrow + g.rrow <= 4 * 4 * 64 * g.waves && g.w % 4 == 0 && c.aligned4);
        }
        const int asked = c.s.opt.cost_workgroup_waves;
        if (k == 0 && (asked == 1 || asked == 2 || asked == 4)) EXPECT(g.waves == asked || g.lrow + g.rrow <= 4 * 4 * 64 * g.waves);
        if (k == 1) EXPECT(g.waves == 1);
        if (c.s.opt.cost_tile_h > 0) EXPECT(g.tile_h <= std::min(c.s.opt.cost_tile_h, g.h));
    }
}

static int sweep()
{
    PlanLcg r(0x7377656570ull);
    const int cases = 20000;
    for (int i = 0; i < cases; i++) {
        const PlanCase c = plan_sweep_case(r);
        check_match(c);
        check_cost(c);
    }
    printf("cases=%d failures=%d\n", cases, failures);
    return failures ? 1 : 0;
}

static int time_cost()
{
    const std::vector<PlanCase> cases = plan_cost_cases();
    for (int k = 0; k < 3; k++) {
        printf("model %s ns/call:", COST_NAMES[k]);
        for (int rep = 0; rep < 5; rep++) {
            long long sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < 100000; i++) {
                const PlanCase &c = cases[i % cases.size()];
                SadGeom q;
                q.lds_bytes = 0;
                if (COST_PLANNERS[k](c.s, c.pairs, c.aligned4 != 0, &q).family) sink += q.lds_bytes;
            }
            const auto t1 = std::chrono::steady_clock::now();
            printf(" %.1f", std::chrono::duration<double, std::nano>(t1 - t0).count() / 100000.0);
            if (sink == 42) printf("!");
        }
        printf("\n");
    }
    return 0;
}

// The strip kernel k_cost_strip<half, SSD, NS> runs behind a fast cost kernel on a ghost-border plan, NS = 1 up to 256
// shifts and 2 beyond (sm_cost_wta, sm_cost_strip_launch).  Every window and shift count the cost mode accepts, on a few
// sizes, batch sizes, alignments and workgroup widths, planned in sm_cost_wta's order: SAD by k_sad_pc, else k_sad_qs;
// SSD by k_ssd_mfma.  Whatever this does not print, no plan launches (tests/golden/kernel_waivers.json).
static int strips()
{
    bool reached[11][2][3] = {};
    for (int n = 1; n <= 25; n += 2)
        for (int D = 1; D <= 1100; D++)
            for (const auto &sz : PLAN_SIZES)
                for (int pairs : {1, 8, 64})
                    for (int aligned4 = 0; aligned4 < 2; aligned4++)
                        for (int waves : {0, 1, 2, 4}) {
                            PlanCase c = plan_case(sz[0], sz[1], D, n, SM_GHOST, pairs, 256);
                            c.s.opt.cost_workgroup_waves = waves;
                            const int half = c.s.square_width / 2;
                            if (half < 1 || half > 10) continue;
                            SadGeom q;
                            bool sad = sm_plan_sad_pc(c.s, pairs, aligned4 != 0, &q).family != SM_COST_KERNEL_NONE;
                            if (!sad) sad = sm_plan_sad_qs(c.s, pairs, aligned4 != 0, &q).family != SM_COST_KERNEL_NONE;
                            const bool ssd = sm_plan_ssd_mfma(c.s, pairs, aligned4 != 0, &q).family != SM_COST_KERNEL_NONE;
                            const int ns = (D + 255) / 256;
                            if (ns > 2) { if (sad || ssd) return 1; continue; }       // (sm_cost_strip_launch refuses it)
                            reached[half][0][ns] |= sad;
                            reached[half][1][ns] |= ssd;
                        }
    for (int half = 1; half <= 10; half++)
        for (int ssd = 0; ssd < 2; ssd++)
            for (int ns = 1; ns <= 2; ns++)
                if (reached[half][ssd][ns]) printf("k_cost_strip<%d, %s, %d>\n", half, ssd ? "true" : "false", ns);
    return 0;
}

int main(int argc, char **argv)
{
    const char *mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "dump")) return dump();
    if (!strcmp(mode, "sweep")) return sweep();
    if (!strcmp(mode, "stats")) return stats();
    if (!strcmp(mode, "time")) return time_cost();
    if (!strcmp(mode, "strips")) return strips();
    if (!strcmp(mode, "case") && argc == 4) {
        const std::vector<PlanCase> cases = atoi(argv[2]) ? plan_cost_cases() : plan_match_cases();
        const size_t i = (size_t)atoi(argv[3]);
        if (i >= cases.size()) return 2;
        print_case(cases[i]);
        return 0;
    }
    fprintf(stderr, "usage: plan_model_check dump | sweep | stats | time | strips | case K N\n");
    return 2;
}
