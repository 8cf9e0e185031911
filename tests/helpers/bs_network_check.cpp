// bs_network_check.cpp -- the signed carry-save network of csrc/sm_bs_network.h, built for the
// host (bop<IMM> in plain C++) and run against integer arithmetic.
//
//   bs_network_check counts     one line per window: N SB network_ops separate_ops cells
//   bs_network_check check      every window the library instantiates; prints the number of
//                               cases per window, exits 1 at the first wrong sum
//
// A call updates IT = 4 sums side by side, and each of the 32 bit positions of a word is a case
// of its own: 128 cases per call.  Legal cases only: 0 <= S, S' <= N * N.
#define SM_BS_NETWORK_HOST
#include "sm_bs_network.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

struct Case { uint32_t e, l; int s; };      // entering bits, leaving bits, S

template <int N>
struct Runner {
    static constexpr int SB = bits_for(N * N), IT = 4, NN = N * N;
    std::vector<Case> pending;
    long long ncases = 0;

    static int popc(uint32_t v) { return __builtin_popcount(v); }
    // the nearest legal S: 0 <= S <= N^2 and 0 <= S + #e - #l <= N^2
    static int legal(int s, uint32_t e, uint32_t l)
    {
        const int d = popc(l) - popc(e);
        const int lo = d > 0 ? d : 0, hi = d < 0 ? NN + d : NN;
        return s < lo ? lo : s > hi ? hi : s;
    }
    void add(uint32_t e, uint32_t l, int s)
    {
        pending.push_back({e, l, legal(s, e, l)});
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
            for (int i = 0; i < N; i++) {
                x[it][i] |= ((k.e >> i) & 1u) << bit;
                x[it][N + i] |= ((k.l >> i) & 1u) << bit;
            }
            for (int p = 0; p < SB; p++) S[it][p] |= (uint32_t)((k.s >> p) & 1) << bit;
        }
        network_lockstep<N, SB, IT, IT>(S, 0, [&](int it, int i) -> u32 { return x[it][i]; });
        for (int c = 0; c < n; c++) {
            const int it = c >> 5, bit = c & 31;
            const Case &k = pending[c];
            int got = 0;
            for (int p = 0; p < SB; p++) got |= (int)((S[it][p] >> bit) & 1u) << p;
            const int want = k.s + popc(k.e) - popc(k.l);
            if (want < 0 || want > NN) { printf("N=%d: the generator made an illegal case\n", N); exit(2); }
            if (got != want) {
                printf("N=%d: e=%#x l=%#x S=%d: got %d, want %d\n", N, k.e, k.l, k.s, got, want);
                exit(1);
            }
        }
        ncases += n;
        pending.clear();
    }
    void with_s_set(uint32_t e, uint32_t l, int nrandom)
    {
        const int d = popc(l) - popc(e);
        add(e, l, 0); add(e, l, 1); add(e, l, d);            // d: S' = 0
        add(e, l, NN - 1); add(e, l, NN);
        const int lo = d > 0 ? d : 0, hi = d < 0 ? NN + d : NN;
        for (int r = 0; r < nrandom; r++) add(e, l, lo + (int)(rng() % (uint64_t)(hi - lo + 1)));
    }
    void run()
    {
        const uint32_t all = (1u << N) - 1u;
        if (N <= 9) {
            // every combination of entering and leaving bits
            for (uint32_t e = 0; e <= all; e++)
                for (uint32_t l = 0; l <= all; l++) with_s_set(e, l, 64);
        } else {
            for (int r = 0; r < 1000000; r++) {
                const uint32_t e = (uint32_t)rng() & all, l = (uint32_t)rng() & all;
                const int d = popc(l) - popc(e);
                const int lo = d > 0 ? d : 0, hi = d < 0 ? NN + d : NN;
                add(e, l, lo + (int)(rng() % (uint64_t)(hi - lo + 1)));
            }
        }
        // corners: everything enters an empty window, everything leaves a full one, and ties
        // (as many enter as leave) at the ends and inside
        with_s_set(all, 0, 64);
        add(all, 0, 0);
        with_s_set(0, all, 64);
        add(0, all, NN);
        for (int r = 0; r < 4096; r++) {
            const uint32_t e = (uint32_t)rng() & all;
            uint32_t l = 0;                              // the same number of bits, elsewhere
            for (int k = popc(e); k > 0;) { const uint32_t b = 1u << (rng() % N); if (!(l & b)) { l |= b; k--; } }
            with_s_set(e, l, 4);
            with_s_set(e, e, 1);
        }
        with_s_set(0, 0, 64);
        with_s_set(all, all, 64);
        flush();
        printf("N=%d SB=%d cases=%lld ok\n", N, SB, ncases);
    }
};

template <int N>
static void counts()
{
    constexpr int SB = bits_for(N * N);
    constexpr NetPlan<N, SB> P = NetPlanOf<N, SB>::value;
    printf("%d %d %d %d %d\n", N, SB, net_ops<N>(), net_ops_separate(N), P.ncell);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "counts")) {
        counts<3>(); counts<5>(); counts<7>(); counts<9>(); counts<11>(); counts<13>();
        counts<15>(); counts<17>(); counts<19>(); counts<21>();
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "check")) {
        Runner<3>().run(); Runner<5>().run(); Runner<7>().run(); Runner<9>().run(); Runner<11>().run(); Runner<13>().run();
        Runner<15>().run(); Runner<17>().run(); Runner<19>().run(); Runner<21>().run();
        return 0;
    }
    fprintf(stderr, "usage: %s counts|check\n", argv[0]);
    return 2;
}
