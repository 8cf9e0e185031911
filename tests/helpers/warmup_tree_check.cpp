// warmup_tree_check.cpp -- the counter of a two-wave workgroup's shared warm-up rows (count_chain_lockstep of
// csrc/sm_bs_network.h: HALF * N one-bit inputs to their count on bits_for(HALF * N) planes), built for the host and
// run against integer popcounts.
//
//   warmup_tree_check counts     one line per window: N NI TB tree_ops rows_ops cells
//   warmup_tree_check check      every window whose two-wave builds take the counter (5 x 5 ... 13 x 13, warm_tree_taken
//                                of csrc/sm_match_bs_kernel.h); prints the number of cases per window, exits 1 at the
//                                first wrong count
//   warmup_tree_check sampled    the same, exhaustive only up to 10 inputs and with 10^5 random patterns per window
//                                (for the build with sanitizers, whose instrumented counter is ~50 times slower)
//
// A call counts IT = 4 items side by side, as the kernel does, and each of the 32 bit positions of a word is a case
// of its own: 128 cases per call.  Every pattern goes through a second pass with IT = 2, the fewest items the
// lockstep form is written for (the kernel's GW is 4 at every DS it is built for).  Per window:
//   * NI <= 21 (5 x 5, 7 x 7): every one of the 2^NI input patterns;
//   * above: every pattern of weight <= 2 and >= NI - 2 (all-zero and all-one among them), and 10^6 random
//     patterns (xorshift64 from the seed 0x9E3779B97F4A7C15), every fourth of them thinned or filled so that low
//     and high counts are sampled as well.
#define SM_BS_NETWORK_HOST
#include "sm_bs_network.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const uint64_t SEED = 0x9E3779B97F4A7C15ull;
static uint64_t rng_state = SEED;
static inline uint64_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// the written operation counts of the kernel's comment: 36 mismatch bits + 68 adder operations in one counter
// against 4 rows of 9 + 14 + 13
static_assert(warm_ops_tree<9>() == 104 && warm_ops_rows(9) == 144, "operations per shift at 9 x 9");
static_assert(warm_ops_tree<9>() - 36 == 2 * (36 - bits_for(36)) + 8, "68: two per full adder, and four half adders and a top wire");

template <int N>
struct Runner {
    static constexpr int HALF = N / 2, NI = HALF * N, TB = bits_for(NI), W = (NI + 63) / 64;
    struct Pattern { uint64_t w[W]; };
    std::vector<Pattern> pending;
    long long ncases = 0;

    static int weight(const Pattern &p) { int c = 0; for (int k = 0; k < W; k++) c += __builtin_popcountll(p.w[k]); return c; }
    static bool bit(const Pattern &p, int i) { return (p.w[i >> 6] >> (i & 63)) & 1u; }
    static Pattern none() { Pattern p; memset(&p, 0, sizeof p); return p; }
    static Pattern all() { Pattern p = none(); for (int i = 0; i < NI; i++) p.w[i >> 6] |= 1ull << (i & 63); return p; }
    static Pattern flip(Pattern p, int i) { p.w[i >> 6] ^= 1ull << (i & 63); return p; }

    template <int IT>
    void flush_it()
    {
        const int n = (int)pending.size();
        for (int c0 = 0; c0 < n; c0 += 32 * IT) {
            const int m = n - c0 < 32 * IT ? n - c0 : 32 * IT;
            uint32_t x[IT][NI], h[IT][TB];
            memset(x, 0, sizeof x);
            for (int c = 0; c < m; c++)
                for (int i = 0; i < NI; i++) x[c >> 5][i] |= (uint32_t)bit(pending[c0 + c], i) << (c & 31);
            count_chain_lockstep<NI, TB, IT>([&](int it, int i) -> u32 { return x[it][i]; }, h);
            for (int c = 0; c < m; c++) {
                int got = 0;
                for (int p = 0; p < TB; p++) got |= (int)((h[c >> 5][p] >> (c & 31)) & 1u) << p;
                const int want = weight(pending[c0 + c]);
                if (got != want) {
                    printf("N=%d IT=%d: pattern", N, IT);
                    for (int k = W - 1; k >= 0; k--) printf(" %016llx", (unsigned long long)pending[c0 + c].w[k]);
                    printf(": got %d, want %d\n", got, want);
                    exit(1);
                }
            }
        }
    }
    void flush()
    {
        flush_it<4>();
        flush_it<2>();
        ncases += (long long)pending.size();
        pending.clear();
    }
    void add(const Pattern &p)
    {
        pending.push_back(p);
        if (pending.size() == 4096) flush();
    }
    void run(bool sampled)
    {
        if (NI <= (sampled ? 10 : 21)) {
            for (uint64_t v = 0; v < (1ull << (NI & 31)); v++) { Pattern p = none(); p.w[0] = v; add(p); }
        } else {
            // weight 0, 1, 2 and NI, NI - 1, NI - 2
            add(none()); add(all());
            for (int i = 0; i < NI; i++) {
                add(flip(none(), i)); add(flip(all(), i));
                for (int j = i + 1; j < NI; j++) { add(flip(flip(none(), i), j)); add(flip(flip(all(), i), j)); }
            }
            for (int r = 0, nr = sampled ? 100000 : 1000000; r < nr; r++) {
                Pattern p = none(), a = all();
                for (int k = 0; k < W; k++) {
                    p.w[k] = rng() & a.w[k];
                    if ((r & 3) == 1) p.w[k] &= rng() & rng();            // sparse
                    if ((r & 3) == 3) p.w[k] |= (rng() | rng()) & a.w[k];  // dense
                }
                add(p);
            }
        }
        flush();
        printf("N=%d NI=%d TB=%d cases=%lld seed=%#llx ok\n", N, NI, TB, ncases, (unsigned long long)SEED);
    }
};

template <int N>
static void counts()
{
    constexpr int NI = N / 2 * N, TB = bits_for(NI);
    constexpr CountPlan<NI, TB> P = CountPlanOf<NI, TB>::value;
    static_assert(count_min_distance<NI, TB>(4) >= 4, "dependency distance, four shifts side by side");
    static_assert(count_min_distance<NI, TB>(2) >= 2, "dependency distance, two shifts side by side");
    static_assert(warm_ops_tree<N>() < warm_ops_rows(N), "the counter is the shorter form");
    printf("%d %d %d %d %d %d\n", N, NI, TB, warm_ops_tree<N>(), warm_ops_rows(N), P.ncell);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "counts")) {
        counts<5>(); counts<7>(); counts<9>(); counts<11>(); counts<13>();
        return 0;
    }
    if (argc == 2 && (!strcmp(argv[1], "check") || !strcmp(argv[1], "sampled"))) {
        const bool q = !strcmp(argv[1], "sampled");
        Runner<5>().run(q); Runner<7>().run(q); Runner<9>().run(q); Runner<11>().run(q); Runner<13>().run(q);
        return 0;
    }
    fprintf(stderr, "usage: %s counts|check|sampled\n", argv[0]);
    return 2;
}
