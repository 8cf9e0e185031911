// sm_cross.hip -- cross-based adaptive support over the census cost: arms that follow the reference image, span sums
// of the Hamming cost over them, first-minimum arg-min, the right-reference pass and the check, and the equiangular
// subpixel fit (include/stereo_hip.h).
//
// PARITY UNPINNED, like census: the reference has no such mode.  Definition (tests/cross_reference.py):
//   a_dir(p), dir in left, right, up, down: the largest l in 0 .. L such that every k = 1 .. l has p + k dir inside
//   the image and |I(p + k dir) - I(p)| <= tau; packed l | r << 4 | u << 8 | d << 12;
//   N(x, y)   = sum over y' = y - u(x, y) .. y + d(x, y) of l(x, y') + r(x, y') + 1                    (N <= 961)
//   c_d       = sm_census.hip's: popcount(C_L(x, y) ^ C_R(x + d, y)) (toroidal: x + d mod W; ghost: C_R = 0 past W)
//   H_d(x, y) = sum over x' = x - l(x, y) .. x + r(x, y) of c_d(x', y)          arms of the pass's reference image
//   E_d(x, y) = sum over y' = y - u(x, y) .. y + d(x, y) of H_d(x, y')          E <= 48 * 961 = 46128 < 2^16
//   best = min_d E_d, web = 1 + the first d reaching it.  The plan's square_width plays no part.
//
// Kernels:
//   k_cross_arms    the arms of a batch of images, a 64 x 16 tile per workgroup from gray rows staged in LDS with a
//                   halo of 15; optionally N, from the horizontal arms of the 15 rows above and below as well.
//   k_cross_wta     the costs, both span sums and the arg-min; no buffer grows with D.  A workgroup of four waves owns
//                   64 - 2 L output columns x 32 rows; a wave's 64 lanes are the 64 columns of the tile with its halo, so
//                   a ROW prefix sum is a scan across the wave and H = P[x + r] - P[x - l - 1] two lane reads.  Eight
//                   shifts a turn, as four packed pairs (u16 | u16: P <= 64 * 48): every wave computes H of its rows
//                   (one in four of the 32 + 2 L) for the four pairs
//                   into LDS; then wave k walks pair k down the columns, overwriting H with its COLUMN prefix sum Q and
//                   reading E = Q[y + d] - Q[y - u - 1] for its 32 output rows into running keys E << 16 | d.  Q passes
//                   2^16 (62 rows of H <= 1488): its halves are summed modulo 2^16 (v_pk_add_u16), and the difference
//                   is exact because E < 2^16.  The keys of the four waves are merged through LDS at the end.  MIRROR:
//                   the right-reference pass, the left pass over mirror(R), mirror(L): descriptors as k_census_wta reads
//                   them, the arms of the right image in mirrored order with l and r exchanged, maps in natural order.
//   k_cross_refine  the three costs E(s-2), E(s-1), E(s) of each pixel tap by tap over its support, and sm_cost_refine's
//                   equiangular fit.

#include "sm_device.h"
#include "sm_census.h"

typedef uint16_t u16;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

#define SMX_ARM 15         // the longest arm
#define SMX_TX 64          // arms: columns per workgroup
#define SMX_TR 16          // arms: rows per workgroup (4 per lane)
#define SMX_TH 32          // wta: output rows per workgroup
#define SMX_DS 8           // wta: shifts a turn (four packed pairs, one per wave in the column walk)

// ---------------------------------------------------------------------------
// arms
// ---------------------------------------------------------------------------

// Images z < n_a come from src_a and go to dst + z * W * H; the others from src_b, to dst + dst_b + (z - n_a) * W * H.
// Workgroup 64 x 4 threads, a tile of 64 columns x 16 rows.  support: NULL, or N of the images (same layout as dst).
__global__ __launch_bounds__(256) void k_cross_arms(const u8 *__restrict__ src_a, const u8 *__restrict__ src_b, int n_a,
                                                    u16 *__restrict__ dst, long long dst_b, i32 *__restrict__ support,
                                                    int W, int H, int tau, int L)
{
    constexpr int SW = SMX_TX + 2 * SMX_ARM, SH = SMX_TR + 2 * SMX_ARM;
    __shared__ u8 tile[SH][SW + 2];
    __shared__ u8 span[SH][SMX_TX];                       // l | r << 4 of the tile's columns, halo rows included
    const int z = blockIdx.z;
    const bool b = z >= n_a;
    const size_t npx = (size_t)W * H;
    const u8 *src = b ? src_b + (size_t)(z - n_a) * npx : src_a + (size_t)z * npx;
    const size_t img = (b ? (size_t)dst_b : 0) + (size_t)(b ? z - n_a : z) * npx;
    const int x0 = blockIdx.x * SMX_TX, y0 = blockIdx.y * SMX_TR;
    const int tid = threadIdx.y * SMX_TX + threadIdx.x;
    // (arms never leave the image: a position outside it is never compared, so it holds the nearest pixel)
    for (int i = tid; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const int x = min(max(x0 - SMX_ARM + c, 0), W - 1), y = min(max(y0 - SMX_ARM + r, 0), H - 1);
        tile[r][c] = src[(size_t)y * W + x];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    const bool on = x < W;
    const int c = threadIdx.x + SMX_ARM;
    const int ml = min(L, x), mr = min(L, W - 1 - x);
    // the horizontal arms: of the tile's rows, and for N of the halo rows that lie inside the image
    const int r_lo = support ? 0 : SMX_ARM, r_hi = support ? SH : SMX_ARM + SMX_TR;
    for (int r = r_lo + threadIdx.y; r < r_hi; r += 4) {
        const int y = y0 - SMX_ARM + r;
        int l = 0, rr = 0;
        if (on && y >= 0 && y < H) {
            const int v = tile[r][c];
            while (l < ml && abs((int)tile[r][c - l - 1] - v) <= tau) l++;
            while (rr < mr && abs((int)tile[r][c + rr + 1] - v) <= tau) rr++;
        }
        span[r][threadIdx.x] = (u8)(l | rr << 4);
    }
    __syncthreads();
    if (!on) return;
#pragma unroll
    for (int q = 0; q < SMX_TR / 4; q++) {
        const int ry = threadIdx.y + 4 * q;
        const int y = y0 + ry;
        if (y >= H) break;
        const int r = ry + SMX_ARM;
        const int v = tile[r][c];
        const int mu = min(L, y), md = min(L, H - 1 - y);
        int u = 0, d = 0;
        while (u < mu && abs((int)tile[r - u - 1][c] - v) <= tau) u++;
        while (d < md && abs((int)tile[r + d + 1][c] - v) <= tau) d++;
        const size_t o = img + (size_t)y * W + x;
        dst[o] = (u16)(span[r][threadIdx.x] | u << 8 | d << 12);
        if (support) {
            int n = 0;
            for (int k = r - u; k <= r + d; k++) n += (span[k][threadIdx.x] & 15) + (span[k][threadIdx.x] >> 4) + 1;
            support[o] = n;
        }
    }
}

// ---------------------------------------------------------------------------
// cost, span sums, arg-min
// ---------------------------------------------------------------------------

struct CrossGeom {
    int w, h, D;
    int arm;                // L: the halo of a tile
    int tw;                 // output columns per workgroup: 64 - 2 L
    int sh;                 // rows of a tile with its halo: 32 + 2 L
    int tiles_x, tiles_y;
    long long side;         // pixels from side 0 (left) to side 1 (right) of the descriptors and of the arms
};

// inclusive sum over the lanes below and the lane itself (the halves of v cannot carry: 64 * 48 < 2^16)
__device__ __forceinline__ u32 smx_scan(u32 v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 t = (u32)__shfl_up((int)v, off);
        if (lane >= off) v += t;
    }
    return v;
}

template <int NW>
__device__ __forceinline__ u32 smx_hamming(const u32 (&a)[NW], const u32 *b)
{
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) c += (u32)__builtin_popcount(a[k] ^ b[k]);
    return c;
}

template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(256) void k_cross_wta(const u32 *__restrict__ desc, const u16 *__restrict__ arms,
                                                   i32 *__restrict__ web, i32 *__restrict__ best, const CrossGeom g)
{
    extern __shared__ __attribute__((aligned(16))) u32 lds[];   // [4 pairs][sh][64]: H, then Q; at the end [4][32][64] keys
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.z;
    int tx, ty;
    sm_xcd_tile(g.tiles_x, g.tiles_y, tx, ty);
    const int W = g.w, H = g.h, L = g.arm, SH = g.sh;
    const size_t npx = (size_t)W * H;
    const int x = tx * g.tw - L + lane;                   // this lane's column (of the pass)
    const int y0 = ty * SMX_TH - L;                       // image row of the tile's row 0
    const bool xin = x >= 0 && x < W;
    const int xn = MIRROR ? W - 1 - x : x;                // ... in the natural order of the stored images
    const bool out_lane = lane >= L && lane < L + g.tw && x < W;
    // MIRROR: the pass's left image is mirror(R), its right image mirror(L)
    const u32 *dL = desc + (size_t)NW * ((MIRROR ? (size_t)g.side : 0) + (size_t)pair * npx);
    const u32 *dR = desc + (size_t)NW * ((MIRROR ? 0 : (size_t)g.side) + (size_t)pair * npx);
    const u16 *aP = arms + (MIRROR ? (size_t)g.side : 0) + (size_t)pair * npx;

    // ---- the output rows of this lane's column: vertical arms u | d << 4, a byte a row
    u32 ud[SMX_TH / 4] = {};
#pragma unroll
    for (int ry = 0; ry < SMX_TH; ry++) {
        const int y = ty * SMX_TH + ry;
        if (out_lane && y < H) ud[ry >> 2] |= ((u32)aP[(size_t)y * W + xn] >> 8) << (8 * (ry & 3));
    }
    u32 key[SMX_TH];
#pragma unroll
    for (int ry = 0; ry < SMX_TH; ry++) key[ry] = 0xffffffffu;

    for (int dlo = 0; dlo < g.D; dlo += SMX_DS) {
        // ---- row sums H of this wave's rows for the turn's four pairs of shifts
        int xb = 0;                                       // x + dlo under the border rule (toroidal: mod W)
        if (xin) xb = GHOST ? x + dlo : smn_mod(x + dlo, W);
        for (int r = wave; r < SH; r += 4) {
            const int y = y0 + r;
            const bool row_on = y >= 0 && y < H;          // (the same for the whole wave)
            const size_t rowo = (size_t)(row_on ? y : 0) * W;
            // the row's left descriptor and horizontal arms at this lane's column (again every turn: from the caches)
            u32 dl[NW];
#pragma unroll
            for (int k = 0; k < NW; k++) dl[k] = 0;
            int l = 0, rr = 0;
            if (row_on && xin) {
#pragma unroll
                for (int k = 0; k < NW; k++) dl[k] = dL[NW * (rowo + xn) + k];
                const u32 a = aP[rowo + xn];
                l = MIRROR ? (a >> 4 & 15) : (a & 15);
                rr = MIRROR ? (a & 15) : (a >> 4 & 15);
            }
            for (int p = 0; p < SMX_DS / 2; p++) {
                if (dlo + 2 * p >= g.D) break;
                u32 h = 0;
                if (row_on) {
                    u32 c[2] = {0, 0};
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        int xr = xb + 2 * p + j;
                        u32 dr[NW];
#pragma unroll
                        for (int k = 0; k < NW; k++) dr[k] = 0;
                        bool have = xin;
                        if (GHOST) have = have && xr < W;
                        else while (xr >= W) xr -= W;
                        if (have) {
                            const size_t o = rowo + (MIRROR ? W - 1 - xr : xr);
#pragma unroll
                            for (int k = 0; k < NW; k++) dr[k] = dR[NW * o + k];
                        }
                        // (a shift past the range is computed and never read: its key is left out below)
                        c[j] = xin ? smx_hamming<NW>(dl, dr) : 0u;
                    }
                    const u32 P = smx_scan(c[0] | c[1] << 16, lane);
                    const u32 hi = (u32)__shfl((int)P, min(lane + rr, 63));
                    const u32 lo = (u32)__shfl((int)P, max(lane - l - 1, 0));
                    h = hi - (lane - l - 1 >= 0 ? lo : 0u);
                }
                lds[((size_t)p * SH + r) * 64 + lane] = h;
            }
        }
        __syncthreads();
        // ---- wave k: the column sums of pair k, and the keys of its two shifts
        const int d = dlo + 2 * wave;
        if (d < g.D) {
            u32 *col = lds + (size_t)wave * SH * 64 + lane;
            u16x2 q = {0, 0};
            for (int r = 0; r < SH; r++) {
                q += __builtin_bit_cast(u16x2, col[(size_t)r * 64]);      // modulo 2^16 in each half
                col[(size_t)r * 64] = __builtin_bit_cast(u32, q);
            }
            const bool two = d + 1 < g.D;
#pragma unroll
            for (int ry = 0; ry < SMX_TH; ry++) {
                // (every lane and row: one outside the image or the tile's output has arms 0, reads inside the tile,
                // and its key is never written)
                {
                    const int r = L + ry;
                    // (arms are at most L by construction; the bound keeps the reads inside the tile whatever they hold)
                    const int u = min((int)(ud[ry >> 2] >> (8 * (ry & 3)) & 15), L);
                    const int dn = min((int)(ud[ry >> 2] >> (8 * (ry & 3) + 4) & 15), L);
                    const u16x2 hi = __builtin_bit_cast(u16x2, col[(size_t)(r + dn) * 64]);
                    const int rl = r - u - 1;
                    u16x2 lo = {0, 0};
                    if (rl >= 0) lo = __builtin_bit_cast(u16x2, col[(size_t)rl * 64]);
                    const u32 e = __builtin_bit_cast(u32, (u16x2)(hi - lo));      // exact: E < 2^16
                    const u32 k0 = e << 16 | (u32)d, k1 = two ? ((e & 0xffff0000u) | (u32)(d + 1)) : 0xffffffffu;
                    key[ry] = min(key[ry], min(k0, k1));
                }
            }
        }
        __syncthreads();
    }

    // ---- the four waves' keys (of different shifts) through LDS: first-wins, the smaller key
#pragma unroll
    for (int ry = 0; ry < SMX_TH; ry++) lds[((size_t)wave * SMX_TH + ry) * 64 + lane] = key[ry];
    __syncthreads();
    if (!out_lane) return;
#pragma unroll
    for (int j = 0; j < SMX_TH / 4; j++) {
        const int ry = wave * (SMX_TH / 4) + j;
        const int y = ty * SMX_TH + ry;
        if (y >= H) break;
        u32 k = 0xffffffffu;
#pragma unroll
        for (int w4 = 0; w4 < 4; w4++) k = min(k, lds[((size_t)w4 * SMX_TH + ry) * 64 + lane]);
        const size_t o = ((size_t)pair * H + y) * W + xn;
        web[o] = (i32)(k & 0xffff) + 1;
        if (best) best[o] = (i32)(k >> 16);
    }
}

// ---------------------------------------------------------------------------
// subpixel refinement
// ---------------------------------------------------------------------------

// One lane per pixel of the LEFT pass: s = web(x, y); for s in 1..D the costs E(s-2), E(s-1), E(s) summed tap by tap
// over the pixel's support (each tap one left descriptor; its three right descriptors slide along the span).
template <int NW, bool GHOST>
__global__ __launch_bounds__(256) void k_cross_refine(const u32 *__restrict__ desc, const u16 *__restrict__ arms,
                                                      const i32 *__restrict__ web, int16_t *__restrict__ sub,
                                                      const CrossGeom g)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int pair = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const int W = g.w, H = g.h;
    const size_t npx = (size_t)W * H;
    const u32 *dL = desc + (size_t)NW * ((size_t)pair * npx);
    const u32 *dR = desc + (size_t)NW * ((size_t)g.side + (size_t)pair * npx);
    const u16 *aP = arms + (size_t)pair * npx;
    const size_t o = (size_t)pair * npx + (size_t)y * W + x;
    const int s = web[o];
    int16_t out = 0;
    if (s >= 1 && s <= g.D) {
        u32 acc[3] = {0, 0, 0};
        const u32 a = aP[(size_t)y * W + x];
        const int y_lo = max(y - (int)(a >> 8 & 15), 0), y_hi = min(y + (int)(a >> 12 & 15), H - 1);
        for (int yy = y_lo; yy <= y_hi; yy++) {
            const size_t rowo = (size_t)yy * W;
            const u32 ar = aP[rowo + x];
            const int x_lo = max(x - (int)(ar & 15), 0), x_hi = min(x + (int)(ar >> 4 & 15), W - 1);
            auto rload = [&](int xr, u32 (&v)[NW]) {
#pragma unroll
                for (int k = 0; k < NW; k++) v[k] = 0;
                if (GHOST) { if (xr < 0 || xr >= W) return; }
                else xr = smn_mod(xr, W);
#pragma unroll
                for (int k = 0; k < NW; k++) v[k] = dR[NW * (rowo + xr) + k];
            };
            u32 r0[NW], r1[NW], r2[NW], l[NW];
            rload(x_lo + s - 2, r0);
            rload(x_lo + s - 1, r1);
            for (int xx = x_lo; xx <= x_hi; xx++) {
                rload(xx + s, r2);
#pragma unroll
                for (int k = 0; k < NW; k++) l[k] = dL[NW * (rowo + xx) + k];
                acc[0] += smx_hamming<NW>(l, r0);
                acc[1] += smx_hamming<NW>(l, r1);
                acc[2] += smx_hamming<NW>(l, r2);
#pragma unroll
                for (int k = 0; k < NW; k++) { r0[k] = r1[k]; r1[k] = r2[k]; }
            }
        }
        int q = 0;
        if (s >= 2 && s <= g.D - 1) {
            const int ca = (int)acc[0] - (int)acc[1], cb = (int)acc[2] - (int)acc[1];
            const int den = max(ca, cb);
            if (den > 0) q = min(8, max(-8, smn_floordiv(16 * (ca - cb) + den, 2 * den)));
        }
        out = (int16_t)(16 * s + q);
    }
    sub[o] = out;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

extern "C" int sm_plan_reserve_cross(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_cross: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_CROSS, "sm_plan_reserve_cross");
}

// the checks of tau and arm (they need no plan)
static int cross_scalar_args(int tau, int arm, const char *me)
{
    if (tau < 0 || tau > 255) return sm_fail(SM_ERR_ARG, "%s: tau %d outside 0..255", me, tau);
    if (arm < 0 || arm > SMX_ARM) return sm_fail(SM_ERR_ARG, "%s: arm %d outside 0..%d", me, arm, SMX_ARM);
    return SM_OK;
}

// what every matching entry checks besides its pointers (before any device call).  The plan's window plays no part.
static int cross_args(const sm_plan *plan, int census_width, int tau, int arm, int pairs, const char *me)
{
    SM_TRY(sm_check_census_width(census_width, me));
    SM_TRY(cross_scalar_args(tau, arm, me));
    SM_TRY(sm_check_pairs(plan, pairs, me));
    if (plan->num_shifts > 512)
        return sm_fail(SM_ERR_ARG, "%s: built for at most 512 shifts (got %d)", me, plan->num_shifts);
    return SM_OK;
}

static int arms_launch(const sm_plan *plan, const uint8_t *src_a, int images_a, const uint8_t *src_b, int images_b,
                       u16 *dst, long long dst_b, i32 *support, int tau, int arm, hipStream_t st)
{
    int W = plan->width, H = plan->height;
    if (!src_b) src_b = src_a;
    void *args[] = {(void *)&src_a, (void *)&src_b, (void *)&images_a, (void *)&dst, (void *)&dst_b, (void *)&support,
                    (void *)&W, (void *)&H, (void *)&tau, (void *)&arm};
    const dim3 grid((W + SMX_TX - 1) / SMX_TX, (H + SMX_TR - 1) / SMX_TR, images_a + images_b), block(SMX_TX, 4);
    const hipError_t e = hipLaunchKernel((const void *)k_cross_arms, grid, block, args, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_cross_arms failed: %s", hipGetErrorString(e));
    return SM_OK;
}

static CrossGeom cross_geom(const sm_plan *plan, int arm)
{
    CrossGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.arm = arm;
    g.tw = 64 - 2 * arm;
    g.sh = SMX_TH + 2 * arm;
    g.tiles_x = (g.w + g.tw - 1) / g.tw;
    g.tiles_y = (g.h + SMX_TH - 1) / SMX_TH;
    g.side = (long long)plan->max_pairs * g.w * g.h;
    return g;
}

// one direction from the workspace's descriptors and arms; sub (left pass only): the subpixel map of the result
static int cross_pass(const sm_plan *plan, int cw, int arm, bool mirror, int pairs, i32 *d_web, i32 *d_best,
                      int16_t *d_sub, hipStream_t st)
{
    const CrossGeom g = cross_geom(plan, arm);
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = cw == 7 ? SM_PASS_KERNEL(k_cross_wta, 2, ghost, mirror) : SM_PASS_KERNEL(k_cross_wta, 1, ghost, mirror);
    const size_t lds = (size_t)(SMX_DS / 2) * g.sh * 64 * sizeof(u32);      // 62 rows at most: 63488 bytes
    void *args[] = {(void *)&plan->d_census, (void *)&plan->d_cross, (void *)&d_web, (void *)&d_best, (void *)&g};
    hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y, pairs), dim3(256), args, lds, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_cross_wta failed: %s", hipGetErrorString(e));
    if (!d_sub) return SM_OK;
    const void *rf = cw == 7 ? (ghost ? (const void *)k_cross_refine<2, true> : (const void *)k_cross_refine<2, false>)
                             : (ghost ? (const void *)k_cross_refine<1, true> : (const void *)k_cross_refine<1, false>);
    void *rargs[] = {(void *)&plan->d_census, (void *)&plan->d_cross, (void *)&d_web, (void *)&d_sub, (void *)&g};
    e = hipLaunchKernel(rf, dim3((g.w + 63) / 64, (g.h + 3) / 4, pairs), dim3(64, 4), rargs, 0, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_cross_refine failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// the mode as the entry driver sees it (sm_entry.h): census descriptors and the arms of both images once, then a pass a
// direction.  Every output is checked against the images (the arms are read from them after the maps could be written
// in a batch of several launches)
struct CrossMode : sm_mode {
    static constexpr const sm_ws_set &ws = SM_WS_SET_CROSS;
    static constexpr bool overlap_names_maps = false;
    int cw, tau, arm;
    const int16_t *sub;
    CrossMode(int census_width, int tau_, int arm_, const int16_t *sub_) : cw(census_width), tau(tau_), arm(arm_), sub(sub_) {}
    int args(const sm_call &c) const { return cross_args(c.plan, cw, tau, arm, c.pairs, c.me); }
    int apart(const sm_call &c, const i32 *const *outs, int n_outs, const i32 *rejected) const
    {
        const size_t px = (size_t)c.pairs * c.plan->width * c.plan->height, map = px * sizeof(i32);
        for (int k = 0; k <= n_outs + 1; k++) {
            const void *o = k < n_outs ? (const void *)outs[k] : k == n_outs ? (const void *)rejected : (const void *)sub;
            const size_t ob = k < n_outs ? map : k == n_outs ? (size_t)c.pairs * sizeof(i32) : px * sizeof(int16_t);
            if (o && (overlap(o, c.left, ob, px) || overlap(o, c.right, ob, px)))
                return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input image", c.me);
        }
        return SM_OK;
    }
    int prepare(const sm_call &c) const
    {
        SM_TRY(sm_census_descriptors(c.plan, cw, c.left, c.right, c.pairs, c.st));
        const long long side = (long long)c.plan->max_pairs * c.plan->width * c.plan->height;
        return arms_launch(c.plan, c.left, c.pairs, c.right, c.pairs, c.plan->d_cross, side, nullptr, tau, arm, c.st);
    }
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *s) const
    {
        return cross_pass(c.plan, cw, arm, mirror, c.pairs, web, best, s, c.st);
    }
};

extern "C" int sm_cross_arms(sm_plan *plan, const uint8_t *d_gray, int tau, int arm, int images, uint16_t *d_arms,
                             int32_t *d_support, void *stream)
{
    const char *me = "sm_cross_arms";
    if (!d_gray || !d_arms) return sm_fail(SM_ERR_ARG, "%s: NULL argument", me);
    SM_TRY(cross_scalar_args(tau, arm, me));
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (images < 1 || images > 2 * plan->max_pairs)
        return sm_fail(SM_ERR_ARG, "%s: images %d outside 1..%d (2 * max_pairs of the plan)", me, images,
                       2 * plan->max_pairs);
    const size_t px = (size_t)images * plan->width * plan->height;
    if (overlap(d_arms, d_gray, px * sizeof(u16), px) || (d_support && overlap(d_support, d_gray, px * sizeof(i32), px)))
        return sm_fail(SM_ERR_ARG, "%s: an output overlaps the input images", me);
    if (d_support && overlap(d_support, d_arms, px * sizeof(i32), px * sizeof(u16)))
        return sm_fail(SM_ERR_ARG, "%s: d_arms and d_support overlap", me);
    SM_TRY(sm_use_device(plan->device));
    return arms_launch(plan, d_gray, images, nullptr, 0, d_arms, 0, d_support, tau, arm, (hipStream_t)stream);
}

extern "C" int sm_cross_wta(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                            int tau, int arm, int pairs, int32_t *d_web, int32_t *d_best, int16_t *d_sub, void *stream)
{
    return sm_entry_one({"sm_cross_wta", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CrossMode(census_width, tau, arm, d_sub), false, d_web, d_best, d_sub);
}

extern "C" int sm_cross_wta_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                  int census_width, int tau, int arm, int pairs, int32_t *d_web_right,
                                  int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_cross_wta_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CrossMode(census_width, tau, arm, nullptr), true, d_web_right, d_best_right, nullptr);
}

extern "C" int sm_cross_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right, int census_width,
                           int tau, int arm, int pairs, int max_diff, int32_t *d_web, int32_t *d_best,
                           int32_t *d_web_right, int32_t *d_rejected, int16_t *d_sub, void *stream)
{
    return sm_entry_lr({"sm_cross_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                       CrossMode(census_width, tau, arm, d_sub), max_diff, d_web, d_best, d_web_right, d_rejected, d_sub);
}
