// sm_sgm_path_body.h -- the text of SGM's path kernel, included twice by sm_sgm.hip (no include guard):
//   SGM_SECOND 0: k_sgm_path<K, MODE>, token for token the kernel as it stood in sm_sgm.hip;
//   SGM_SECOND 1: k_sgm_path_second<K>, the last direction (MODE = SGM_LAST) with a second reduction for the runner-up
//                 of DESIGN.md 22: web2 / best2 beside web / best / sub, while the totals are still in registers.
// Everything the second reduction needs sits under #if SGM_SECOND.
// grid ceil(lines / 4), block 256: one line per wave
#if SGM_SECOND
template <int K>
__global__ __launch_bounds__(256) void k_sgm_path_second(const u16 *__restrict__ A, i32 *__restrict__ S, i32 *web,
                                                         i32 *best, int16_t *sub, i32 *web2, i32 *best2,
                                                         const SgmPathGeom g)
{
    constexpr int MODE = SGM_LAST;
#else
template <int K, int MODE>
__global__ __launch_bounds__(256) void k_sgm_path(const u16 *__restrict__ A, i32 *__restrict__ S, i32 *web, i32 *best,
                                                  int16_t *sub, const SgmPathGeom g)
{
#endif
    const int lane = threadIdx.x & 63;
    const int line = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= g.lines) return;
    const int W = g.w, H = g.h;
    // the line's first pixel: its predecessor lies outside the image
    int x0, y0;
    if (g.dy == 0) {
        y0 = line; x0 = g.dx > 0 ? 0 : W - 1;
    } else if (g.dx == 0) {
        x0 = line; y0 = g.dy > 0 ? 0 : H - 1;
    } else if (line < W) {
        x0 = line; y0 = g.dy > 0 ? 0 : H - 1;
    } else {
        const int j = line - W + 1;
        x0 = g.dx > 0 ? 0 : W - 1; y0 = g.dy > 0 ? j : H - 1 - j;
    }
    const int lx = g.dx > 0 ? W - x0 : g.dx < 0 ? x0 + 1 : 0x7fffffff;
    const int ly = g.dy > 0 ? H - y0 : g.dy < 0 ? y0 + 1 : 0x7fffffff;
    const int len = min(lx, ly);
    const long long pstep = (long long)g.dy * W + g.dx;          // pixels per step
    const long long p0 = (long long)y0 * W + x0;
    const int dl = lane * K;                                     // this lane's first shift
    const u16 *a0 = A + (size_t)p0 * g.Dp + dl;
    i32 *s0 = S + (size_t)p0 * g.Dp + dl;
    const long long vstep = pstep * g.Dp;

    i32 ar[SGP_PF][K], sr[SGP_PF][K];
    auto load = [&](int i, i32 (&av)[K], i32 (&sv)[K]) {
        SgmVec<K>::load_a(a0 + i * vstep, av);
        if (MODE != SGM_FIRST) SgmVec<K>::load_s(s0 + i * vstep, sv);
    };
#pragma unroll
    for (int j = 0; j < SGP_PF; j++)
        if (j < len) load(j, ar[j], sr[j]);

    i32 L[K];
    i32 m = 0;
    const i32 P1 = g.p1, P2 = g.p2;
    for (int base = 0; base < len; base += SGP_PF) {
#pragma unroll
        for (int j = 0; j < SGP_PF; j++) {
            const int i = base + j;
            if (i >= len) break;
            i32 av[K], sv[K];
#pragma unroll
            for (int k = 0; k < K; k++) { av[k] = ar[j][k]; sv[k] = sr[j][k]; }
            if (i + SGP_PF < len) load(i + SGP_PF, ar[j], sr[j]);
            if (i == 0) {
#pragma unroll
                for (int k = 0; k < K; k++) L[k] = dl + k < g.D ? av[k] : SGM_INF;
            } else {
                i32 lo = __shfl_up(L[K - 1], 1), hi = __shfl_down(L[0], 1);   // L(q, d - 1) of entry 0, L(q, d + 1) of K - 1
                if (lane == 0) lo = SGM_INF;
                if (lane == 63) hi = SGM_INF;
                const i32 jump = m + P2;
                i32 nl[K];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const i32 dm = k == 0 ? lo : L[k - 1], dp = k == K - 1 ? hi : L[k + 1];
                    const i32 t = min(min(L[k], min(dm, dp) + P1), jump);
                    nl[k] = dl + k < g.D ? av[k] + t - m : SGM_INF;
                }
#pragma unroll
                for (int k = 0; k < K; k++) L[k] = nl[k];
            }
            i32 lm = L[0];
#pragma unroll
            for (int k = 1; k < K; k++) lm = min(lm, L[k]);
            m = sgm_wave_min(lm);

            if (MODE == SGM_FIRST) {
                SgmVec<K>::store_s(s0 + i * vstep, L);
            } else if (MODE == SGM_MID) {
                i32 t[K];
#pragma unroll
                for (int k = 0; k < K; k++) t[k] = sv[k] + L[k];
                SgmVec<K>::store_s(s0 + i * vstep, t);
            } else {
                // S <= 8 * 62767 < 2^19: keys S << 8 | d, the first d wins a tie; entries d >= D lose to every real one
                // (S = 8 * 62767 and a padded range: tests/test_census_extremes_gpu.py test_sgm_at_its_u16_and_key_bounds)
                i32 tot[K], key = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    tot[k] = sv[k] + L[k];
                    if (dl + k < g.D) key = min(key, (tot[k] << 8) | (dl + k));
                }
                key = sgm_wave_min(key);
                const int s = (key & 0xff) + 1;
                const i32 b = key >> 8;
                int16_t q16 = (int16_t)(16 * s);
                if (sub && s > 1 && s < g.D) {
                    const i32 sm2 = sgm_pick<K>(tot, (s - 2) / K, (s - 2) % K);
                    const i32 sp = sgm_pick<K>(tot, s / K, s % K);
                    const i32 a = sm2 - b, c = sp - b, den = a + c;
                    int q = 0;
                    if (den > 0) q = min(8, max(-8, smn_floordiv(16 * (a - c) + den, 2 * den)));
                    q16 = (int16_t)(16 * s + q);
                }
#if SGM_SECOND
                // the same keys without the shifts within one of the winner's; 0x7fffffff: no shift is left (D <= 2, or
                // D = 3 and the winner in the middle)
                i32 key2 = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int d = dl + k;
                    if (d < g.D && (u32)(d - s + 2) > 2u) key2 = min(key2, (tot[k] << 8) | d);
                }
                key2 = sgm_wave_min(key2);
                const bool none = key2 == 0x7fffffff;
#endif
                if (lane == 0) {
                    const int x = x0 + i * g.dx, y = y0 + i * g.dy;
                    const size_t o = (size_t)g.map + (size_t)y * W + (g.mirror ? W - 1 - x : x);
                    web[o] = s;
                    if (best) best[o] = b;
                    if (sub) sub[o] = q16;
#if SGM_SECOND
                    web2[o] = none ? 0 : (key2 & 0xff) + 1;
                    if (best2) best2[o] = none ? -1 : key2 >> 8;
#endif
                }
            }
        }
    }
}

