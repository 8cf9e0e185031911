// bs_groups_check.cpp -- the signed carry-save network of csrc/sm_bs_network.h with GROUPED inputs (of every
// three columns of a row side the third input is the parity of the group), built for the host and run against
// integer arithmetic S + (entering bits) - (leaving bits).
//
//   bs_groups_check counts      one line per window: N SB grouped_ops per_bit_ops groups_per_side cells
//   bs_groups_check check       every window the library instantiates; prints the number of cases per
//                               window, exits 1 at the first wrong sum
//   bs_groups_check sampled     the same with 9 x 9 sampled like the larger windows and 10^5 samples per window
//                               (for the build with sanitizers, whose instrumented network is ~50 times slower)
//
// A call updates IT = 4 sums side by side, and each of the 32 bit positions of a word is a case of its own: 128
// cases per call.  Legal cases only: 0 <= S, S' <= N * N.  "Every admissible S" of a pair (e, l) of entering and
// leaving bits is every S in [max(0, #l - #e), min(N^2, N^2 + #l - #e)].
//
// Sampled windows (11 x 11 ... 21 x 21): xorshift64 from the seed 0x9E3779B97F4A7C15, 10^6 pairs (e, l) per window.
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

struct Case { uint32_t e, l; int s; };      // entering bits, leaving bits, S

template <int N>
struct Runner {
    static constexpr int SB = bits_for(N * N), IT = 4, NN = N * N, G = N / 3;
    std::vector<Case> pending;
    long long ncases = 0;

    static int popc(uint32_t v) { return __builtin_popcount(v); }
    static int lo_of(uint32_t e, uint32_t l) { const int d = popc(l) - popc(e); return d > 0 ? d : 0; }
    static int hi_of(uint32_t e, uint32_t l) { const int d = popc(l) - popc(e); return d < 0 ? NN + d : NN; }
    void add(uint32_t e, uint32_t l, int s)
    {
        if (s < lo_of(e, l) || s > hi_of(e, l)) { printf("N=%d: the generator made an illegal case\n", N); exit(2); }
        pending.push_back({e, l, s});
        if ((int)pending.size() == 32 * IT) flush();
    }
    void flush()
    {
        if (pending.empty()) return;
        const int n = (int)pending.size();
        uint32_t S[IT][SB], x[IT][2 * N];
        memset(S, 0, sizeof S); memset(x, 0, sizeof x);
        for (int c = 0; c < n; c++) {
            const int it = c >> 5, bit = c & 31;
            const Case &k = pending[c];
            for (int side = 0; side < 2; side++) {
                const uint32_t v = side ? k.l : k.e;
                for (int i = 0; i < N; i++) {
                    uint32_t b = (v >> i) & 1u;
                    // the third input of a group is the parity of its three columns
                    if (i < 3 * G && i % 3 == 2) b ^= ((v >> (i - 1)) ^ (v >> (i - 2))) & 1u;
                    x[it][side * N + i] |= b << bit;
                }
            }
            for (int p = 0; p < SB; p++) S[it][p] |= (uint32_t)((k.s >> p) & 1) << bit;
        }
        network_lockstep<N, SB, IT, IT, true>(S, 0, [&](int it, int i) -> u32 { return x[it][i]; });
        for (int c = 0; c < n; c++) {
            const int it = c >> 5, bit = c & 31;
            const Case &k = pending[c];
            int got = 0;
            for (int p = 0; p < SB; p++) got |= (int)((S[it][p] >> bit) & 1u) << p;
            const int want = k.s + popc(k.e) - popc(k.l);
            if (got != want) {
                printf("N=%d: e=%#x l=%#x S=%d: got %d, want %d\n", N, k.e, k.l, k.s, got, want);
                exit(1);
            }
        }
        ncases += n;
        pending.clear();
    }
    void every_s(uint32_t e, uint32_t l)
    {
        for (int s = lo_of(e, l), hi = hi_of(e, l); s <= hi; s++) add(e, l, s);
    }
    void run(bool sampled)
    {
        const uint32_t all = (1u << N) - 1u;
        if (N <= (sampled ? 7 : 9)) {
            // every combination of entering and leaving bits, with every admissible S
            for (uint32_t e = 0; e <= all; e++)
                for (uint32_t l = 0; l <= all; l++) every_s(e, l);
        } else {
            for (int r = 0, nr = sampled ? 100000 : 1000000; r < nr; r++) {
                const uint32_t e = (uint32_t)rng() & all, l = (uint32_t)rng() & all;
                const int lo = lo_of(e, l), hi = hi_of(e, l);
                add(e, l, lo + (int)(rng() % (uint64_t)(hi - lo + 1)));
                add(e, l, lo);
                add(e, l, hi);
            }
            // everything enters, everything leaves, nothing moves, and single groups full or empty
            every_s(all, 0); every_s(0, all); every_s(0, 0); every_s(all, all);
            for (int g = 0; g < G; g++) {
                const uint32_t grp = 7u << (3 * g);
                every_s(grp, 0); every_s(0, grp); every_s(all & ~grp, all); every_s(all, all & ~grp);
            }
        }
        flush();
        printf("N=%d SB=%d cases=%lld seed=%#llx ok\n", N, SB, ncases, (unsigned long long)SEED);
    }
};

template <int N>
static void counts()
{
    constexpr int SB = bits_for(N * N);
    constexpr NetPlan<N, SB> P = NetPlanOf<N, SB, true>::value;
    static_assert(net_ops<N, true>() == net_ops<N>() - 2 * (N / 3), "one operation fewer per group of three columns");
    static_assert(net_min_distance<N, SB, true>(4) >= 4, "dependency distance of the grouped plan, four shifts side by side");
    int groups = 0;
    for (int i = 0; i < P.ncell; i++) groups += P.cell[i].grp;
    printf("%d %d %d %d %d %d\n", N, SB, net_ops<N, true>(), net_ops<N>(), groups / 2, P.ncell);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "counts")) {
        counts<3>(); counts<5>(); counts<7>(); counts<9>(); counts<11>(); counts<13>();
        counts<15>(); counts<17>(); counts<19>(); counts<21>();
        return 0;
    }
    if (argc == 2 && (!strcmp(argv[1], "check") || !strcmp(argv[1], "sampled"))) {
        const bool q = !strcmp(argv[1], "sampled");
        Runner<3>().run(q); Runner<5>().run(q); Runner<7>().run(q); Runner<9>().run(q); Runner<11>().run(q); Runner<13>().run(q);
        Runner<15>().run(q); Runner<17>().run(q); Runner<19>().run(q); Runner<21>().run(q);
        return 0;
    }
    fprintf(stderr, "usage: %s counts|check|sampled\n", argv[0]);
    return 2;
}
