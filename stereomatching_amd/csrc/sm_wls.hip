// sm_wls.hip -- confidence-weighted edge-aware smoother (include/stereo_hip.h "edge-aware smoother", DESIGN.md section
// 25): the fast global smoother of Min et al. (TIP 2014), used the way OpenCV's DisparityWLSFilter uses it.  The one
// post-filter that is global (a value travels any distance within its surface), that weighs a pixel by sm_confidence's
// byte, and whose result is a dense subpixel map: matcher (+ runner-up) -> confidence -> check -> speckle -> smoother
// -> reproject.
//
// PARITY UNPINNED: the reference has no such stage.  Definition (tests/wls_reference.py is its executable form; the
// header has it in full).  u = 16 v (int32 map) or v (int16 map); c = conf where in != 0, else 0; N = c u, M = c.
// For t = 0 .. T - 1, lambda_t = ((1.5 lambda) 4^(T-1-t)) / (4^T - 1.0): every row, then every column, of N and M is
// replaced by the solution U of the tridiagonal system of its line f_0 .. f_(n-1):
//   links l_i = lambda_t * (double)weights[|g_i - g_(i+1)|], l_(-1) = l_(n-1) = 0
//   a_i = -l_(i-1), k_i = -l_i, b_i = (1.0 + l_(i-1)) + l_i
//   forward:  den_i = b_i - cp_(i-1) a_i, inv_i = 1.0 / den_i, cp_i = k_i inv_i, f'_i = (f_i - f'_(i-1) a_i) inv_i
//             (i = 0: den_0 = b_0, f'_0 = f_0 inv_0)
//   backward: U_(n-1) = f'_(n-1), U_i = f'_i - cp_i U_(i+1)
// every operation an IEEE double operation rounded on its own (the library is built with -ffp-contract=off, and a
// double division is correctly rounded), so the result equals the numpy definition bit for bit.  r = N / M where
// M > 0, else 0; out = rint(r) (int16) or rint(r / 16) (int32), saturated.
//
// Kernels (a line is serial; the parallelism is across lines and pairs, and what is left to design is the memory access):
//   k_wls_init<T>     element-wise: N and M from the map and the confidence.
//   k_wls_cols_fwd    a lane owns a column: 64 adjacent columns are a wave, a workgroup is ONE wave (4K's 60 waves
//   k_wls_cols_bwd    spread over 60 CUs), blockIdx.z the pair.  Every access is a contiguous 512-byte row segment per
//                     plane.  A lane's chain cannot hide a load, so rows travel in batches of WLS_R: the next batch's
//                     loads are issued before this batch is solved.  Forward writes cp and overwrites N and M with
//                     f'; backward reads them back.  The links' table, lambda_t * weights[d] as 256 doubles, is made
//                     once per workgroup in LDS from the table in the kernel's arguments.
//   k_wls_rows_fwd    a lane owns a row, 64 rows a wave.  Direct access would be a stride of W doubles per lane, so
//   k_wls_rows_bwd    chunks of 64 rows x WLS_C columns of N, M (and cp) go through LDS: global loads and stores run
//                     along rows (16 lanes on 128 contiguous bytes), the solve reads down a column of the tile.  The
//                     tile's row stride is WLS_C + 1 doubles = 34 dwords: the 32 lanes of a ds_read_b64 group fall on 32
//                     different even banks of 64.  The guide bytes of the chunk (of the NEXT column: a link needs both
//                     ends) are staged the same way, 20 bytes a row (5 dwords, odd).  The next chunk's global loads are
//                     in flight, in registers, while this one is solved.
//   k_wls_finish<T>   the quotient, the rounding, the optional raw plane and the filled count (lr_count's pattern).
// Every sweep's inner block exists twice: a straight one without a test per step, taken where the batch or chunk and
// its next element are inside (the compiler then moves the next steps' reads above this step's chain), and a guarded
// one for the edges.
// The three chains of a line (cp, N, M) are independent: the only instruction-level parallelism a lane has.  The cp
// chain depends on the guide alone and is computed once per sweep for both planes.  Passes are ordered by the stream.

#include "sm_device.h"

#include <algorithm>
#include <math.h>

#define WLS_MAX_T 8
#define WLS_C 16                    // columns of a row-kernel chunk
#define WLS_LD (WLS_C + 1)          // row stride of its LDS tiles, in doubles
#define WLS_GLD (WLS_C + 4)         // row stride of its guide tile, in bytes
#define WLS_R 8                     // rows of a column-kernel batch

// the links of this sweep by gray difference, in LDS: lw[d] = lambda_t * (double)weights[d] (block of 64)
__device__ __forceinline__ void wls_links(double *lw, const WmedTable &table, double lam)
{
    for (int i = threadIdx.x; i < 256; i += 64) lw[i] = lam * (double)table.w[i];
    __syncthreads();
}

// one forward step: the cp chain, then both planes.  first: i = 0
__device__ __forceinline__ void wls_step(bool first, double lp, double ln, double &cp, double &fn, double &fm, double n, double m)
{
    const double a = -lp, k = -ln, b = (1.0 + lp) + ln;
    const double den = first ? b : b - cp * a;
    const double inv = 1.0 / den;
    const double tn = first ? n : n - fn * a, tm = first ? m : m - fm * a;
    cp = k * inv;
    fn = tn * inv;
    fm = tm * inv;
}

// grid ceil(n / 256), block 256; n = pairs * W * H.  conf: NULL = 255 everywhere
template <typename T>
__global__ __launch_bounds__(256) void k_wls_init(const T *__restrict__ in, const u8 *__restrict__ conf, double *__restrict__ N,
                                                  double *__restrict__ M, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T v = in[i];
    const double u = sizeof(T) == 4 ? 16.0 * (double)v : (double)v;
    const double c = v != 0 ? (conf ? (double)conf[i] : 255.0) : 0.0;
    N[i] = c * u;
    M[i] = c;
}

// grid (ceil(W / 64), 1, pairs), block 64; H >= 2
__global__ __launch_bounds__(64) void k_wls_cols_fwd(const u8 *__restrict__ guide, WmedTable table, double lam,
                                                     double *__restrict__ N, double *__restrict__ M,
                                                     double *__restrict__ CP, int W, int H)
{
    __shared__ double lw[256];
    wls_links(lw, table, lam);
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.z * W * H + x;
    double nn[WLS_R] = {}, nm[WLS_R] = {}, cn[WLS_R], cm[WLS_R];
    int ng[WLS_R] = {}, cg[WLS_R];                       // the guide of the row BELOW
    int gp = guide[base];
#pragma unroll
    for (int j = 0; j < WLS_R; j++)
        if (j < H) {
            nn[j] = N[base + (size_t)j * W];
            nm[j] = M[base + (size_t)j * W];
            ng[j] = j + 1 < H ? guide[base + (size_t)(j + 1) * W] : 0;
        }
    double lp = 0.0, cp = 0.0, fn = 0.0, fm = 0.0;
    for (int r0 = 0; r0 < H; r0 += WLS_R) {
#pragma unroll
        for (int j = 0; j < WLS_R; j++) { cn[j] = nn[j]; cm[j] = nm[j]; cg[j] = ng[j]; }
#pragma unroll
        for (int j = 0; j < WLS_R; j++) {
            const int row = r0 + WLS_R + j;
            if (row < H) {
                nn[j] = N[base + (size_t)row * W];
                nm[j] = M[base + (size_t)row * W];
                ng[j] = row + 1 < H ? guide[base + (size_t)(row + 1) * W] : 0;
            }
        }
        auto step = [&](int j, int row, bool link) {
            const double ln = link ? lw[abs(gp - cg[j])] : 0.0;
            wls_step(row == 0, lp, ln, cp, fn, fm, cn[j], cm[j]);
            CP[base + (size_t)row * W] = cp;
            N[base + (size_t)row * W] = fn;
            M[base + (size_t)row * W] = fm;
            lp = ln;
            gp = cg[j];
        };
        if (r0 + WLS_R < H) {                       // the batch and the row below it are inside: one straight block
#pragma unroll
            for (int j = 0; j < WLS_R; j++) step(j, r0 + j, true);
        } else {
#pragma unroll
            for (int j = 0; j < WLS_R; j++)
                if (r0 + j < H) step(j, r0 + j, r0 + j + 1 < H);
        }
    }
}

// grid (ceil(W / 64), 1, pairs), block 64; H >= 2.  Row H - 1 stays (U = f'); rows H - 2 .. 0 from below
__global__ __launch_bounds__(64) void k_wls_cols_bwd(double *__restrict__ N, double *__restrict__ M,
                                                     const double *__restrict__ CP, int W, int H)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.z * W * H + x;
    double nn[WLS_R] = {}, nm[WLS_R] = {}, nc[WLS_R] = {}, cn[WLS_R], cm[WLS_R], cc[WLS_R];
    double un = N[base + (size_t)(H - 1) * W], um = M[base + (size_t)(H - 1) * W];
#pragma unroll
    for (int j = 0; j < WLS_R; j++) {
        const int row = H - 2 - j;
        if (row >= 0) {
            nn[j] = N[base + (size_t)row * W];
            nm[j] = M[base + (size_t)row * W];
            nc[j] = CP[base + (size_t)row * W];
        }
    }
    for (int r0 = H - 2; r0 >= 0; r0 -= WLS_R) {
#pragma unroll
        for (int j = 0; j < WLS_R; j++) { cn[j] = nn[j]; cm[j] = nm[j]; cc[j] = nc[j]; }
#pragma unroll
        for (int j = 0; j < WLS_R; j++) {
            const int row = r0 - WLS_R - j;
            if (row >= 0) {
                nn[j] = N[base + (size_t)row * W];
                nm[j] = M[base + (size_t)row * W];
                nc[j] = CP[base + (size_t)row * W];
            }
        }
        auto step = [&](int j, int row) {
            un = cn[j] - cc[j] * un;
            um = cm[j] - cc[j] * um;
            N[base + (size_t)row * W] = un;
            M[base + (size_t)row * W] = um;
        };
        if (r0 - (WLS_R - 1) >= 0) {
#pragma unroll
            for (int j = 0; j < WLS_R; j++) step(j, r0 - j);
        } else {
#pragma unroll
            for (int j = 0; j < WLS_R; j++)
                if (r0 - j >= 0) step(j, r0 - j);
        }
    }
}

// A chunk of the row kernels: rows y0 .. y0 + 63, columns c0 .. c0 + WLS_C - 1.  Element e = j * 64 + lane of it
// (j = 0 .. WLS_C - 1) is row e / WLS_C, column e % WLS_C: 16 adjacent lanes on one row's 128 bytes.
#define WLS_EACH(j, r, c) \
    _Pragma("unroll") for (int j = 0, r = threadIdx.x / WLS_C, c = threadIdx.x % WLS_C; j < WLS_C; j++, r += 64 / WLS_C)

// grid (ceil(H / 64), 1, pairs), block 64; W >= 2
__global__ __launch_bounds__(64) void k_wls_rows_fwd(const u8 *__restrict__ guide, WmedTable table, double lam,
                                                     double *__restrict__ N, double *__restrict__ M,
                                                     double *__restrict__ CP, int W, int H)
{
    __shared__ double lw[256];
    __shared__ double tn[64 * WLS_LD], tm[64 * WLS_LD], tc[64 * WLS_LD];
    __shared__ u32 tg[64 * WLS_GLD / 4];            // the guide of the column to the RIGHT: tg8[row * WLS_GLD + column]
    u8 *tg8 = (u8 *)tg;
    wls_links(lw, table, lam);
    const int lane = threadIdx.x, y0 = blockIdx.x * 64, y = y0 + lane;
    const size_t base = (size_t)blockIdx.z * W * H;
    double rn[WLS_C] = {}, rm[WLS_C] = {};
    u8 rg[WLS_C] = {};
    WLS_EACH(j, r, c) {
        if (y0 + r < H && c < W) {
            const size_t at = base + (size_t)(y0 + r) * W + c;
            rn[j] = N[at];
            rm[j] = M[at];
            rg[j] = c + 1 < W ? guide[at + 1] : (u8)0;
        }
    }
    int gp = y < H ? guide[base + (size_t)y * W] : 0;
    double lp = 0.0, cp = 0.0, fn = 0.0, fm = 0.0;
    for (int c0 = 0; c0 < W; c0 += WLS_C) {
        WLS_EACH(j, r, c) {
            tn[r * WLS_LD + c] = rn[j];
            tm[r * WLS_LD + c] = rm[j];
            tg8[r * WLS_GLD + c] = rg[j];
        }
        __syncthreads();
        WLS_EACH(j, r, c) {
            const int col = c0 + WLS_C + c;
            if (y0 + r < H && col < W) {
                const size_t at = base + (size_t)(y0 + r) * W + col;
                rn[j] = N[at];
                rm[j] = M[at];
                rg[j] = col + 1 < W ? guide[at + 1] : (u8)0;
            }
        }
        if (y < H) {
            u32 gw[WLS_C / 4];
#pragma unroll
            for (int q = 0; q < WLS_C / 4; q++) gw[q] = tg[lane * (WLS_GLD / 4) + q];
            auto step = [&](int c, bool first, bool link) {
                const int g1 = (int)(gw[c >> 2] >> (8 * (c & 3)) & 255u);
                const double ln = link ? lw[abs(gp - g1)] : 0.0;
                wls_step(first, lp, ln, cp, fn, fm, tn[lane * WLS_LD + c], tm[lane * WLS_LD + c]);
                tc[lane * WLS_LD + c] = cp;
                tn[lane * WLS_LD + c] = fn;
                tm[lane * WLS_LD + c] = fm;
                lp = ln;
                gp = g1;
            };
            if (c0 + WLS_C < W) {                   // the chunk and the column right of it are inside: one straight block
#pragma unroll
                for (int c = 0; c < WLS_C; c++) step(c, c0 + c == 0, true);
            } else {
#pragma unroll
                for (int c = 0; c < WLS_C; c++)
                    if (c0 + c < W) step(c, c0 + c == 0, c0 + c + 1 < W);
            }
        }
        __syncthreads();
        WLS_EACH(j, r, c) {
            const int col = c0 + c;
            if (y0 + r < H && col < W) {
                const size_t at = base + (size_t)(y0 + r) * W + col;
                CP[at] = tc[r * WLS_LD + c];
                N[at] = tn[r * WLS_LD + c];
                M[at] = tm[r * WLS_LD + c];
            }
        }
        __syncthreads();
    }
}

// grid (ceil(H / 64), 1, pairs), block 64; W >= 2.  Column W - 1 stays (U = f'); columns W - 2 .. 0 from the right
__global__ __launch_bounds__(64) void k_wls_rows_bwd(double *__restrict__ N, double *__restrict__ M,
                                                     const double *__restrict__ CP, int W, int H)
{
    __shared__ double tn[64 * WLS_LD], tm[64 * WLS_LD], tc[64 * WLS_LD];
    const int lane = threadIdx.x, y0 = blockIdx.x * 64, y = y0 + lane;
    const size_t base = (size_t)blockIdx.z * W * H;
    const int c_last = (W - 1) / WLS_C * WLS_C;
    double rn[WLS_C] = {}, rm[WLS_C] = {}, rc[WLS_C] = {};
    WLS_EACH(j, r, c) {
        const int col = c_last + c;
        if (y0 + r < H && col < W) {
            const size_t at = base + (size_t)(y0 + r) * W + col;
            rn[j] = N[at];
            rm[j] = M[at];
            rc[j] = CP[at];
        }
    }
    double un = 0.0, um = 0.0;
    for (int c0 = c_last; c0 >= 0; c0 -= WLS_C) {
        WLS_EACH(j, r, c) {
            tn[r * WLS_LD + c] = rn[j];
            tm[r * WLS_LD + c] = rm[j];
            tc[r * WLS_LD + c] = rc[j];
        }
        __syncthreads();
        WLS_EACH(j, r, c) {
            const int col = c0 - WLS_C + c;
            if (y0 + r < H && col >= 0) {           // (c0 is a multiple of WLS_C: col < W)
                const size_t at = base + (size_t)(y0 + r) * W + col;
                rn[j] = N[at];
                rm[j] = M[at];
                rc[j] = CP[at];
            }
        }
        if (y < H) {
            auto step = [&](int c, bool last) {
                const double f_n = tn[lane * WLS_LD + c], f_m = tm[lane * WLS_LD + c], k = tc[lane * WLS_LD + c];
                un = last ? f_n : f_n - k * un;
                um = last ? f_m : f_m - k * um;
                tn[lane * WLS_LD + c] = un;
                tm[lane * WLS_LD + c] = um;
            };
            if (c0 + WLS_C < W) {                   // (the chunk is inside and column W - 1 is not in it)
#pragma unroll
                for (int c = WLS_C - 1; c >= 0; c--) step(c, false);
            } else {
#pragma unroll
                for (int c = WLS_C - 1; c >= 0; c--)
                    if (c0 + c < W) step(c, c0 + c == W - 1);
            }
        }
        __syncthreads();
        WLS_EACH(j, r, c) {
            const int col = c0 + c;
            if (y0 + r < H && col < W) {
                const size_t at = base + (size_t)(y0 + r) * W + col;
                N[at] = tn[r * WLS_LD + c];
                M[at] = tm[r * WLS_LD + c];
            }
        }
        __syncthreads();
    }
}

// Grid: x strides over the pixels of one pair (at most SM_LR_BLOCKS workgroups), y = pair; block 256.  in and out may
// be the same map of one type: a lane reads its pixel before it writes it.  filled: NULL or the pairs' counts, zeroed
// before the launch
template <typename T>
__global__ __launch_bounds__(256) void k_wls_finish(const void *in, int in_i16, const double *__restrict__ N,
                                                    const double *__restrict__ M, T *out, double *__restrict__ raw,
                                                    i32 *filled, unsigned npx, int no_fill)
{
    const size_t base = (size_t)blockIdx.y * npx;
    int cnt = 0;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npx; p += gridDim.x * 256u) {
        const size_t at = base + p;
        const bool valid = (in_i16 ? (i32)((const int16_t *)in)[at] : ((const i32 *)in)[at]) != 0;
        const double m = M[at];
        double r = m > 0.0 ? N[at] / m : 0.0;
        if (no_fill && !valid) r = 0.0;
        const double lo = sizeof(T) == 4 ? -2147483648.0 : -32768.0, hi = sizeof(T) == 4 ? 2147483647.0 : 32767.0;
        double s = rint(sizeof(T) == 4 ? r / 16.0 : r);
        s = s < lo ? lo : (s > hi ? hi : s);
        const T res = (T)(i32)s;
        out[at] = res;
        if (raw) raw[at] = r;
        cnt += !valid && res != 0;
    }
    if (filled) lr_count(filled + blockIdx.y, cnt);
}

extern "C" int sm_plan_reserve_wls(sm_plan *plan)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_reserve_wls: plan is NULL");
    SM_TRY(sm_use_device(plan->device));
    return sm_ws_reserve(plan, SM_WS_SET_WLS, "sm_plan_reserve_wls");
}

extern "C" int sm_wls_filter(sm_plan *plan, const void *d_in, int map_type, const uint8_t *d_conf, const uint8_t *d_guide,
                             const uint16_t weights[256], double lambda, int iterations, int flags, int pairs, void *d_out,
                             int out_type, double *d_raw, int32_t *d_filled, void *stream)
{
    const char *me = "sm_wls_filter";
    size_t elem, out_elem;
    if (!d_in || !d_out) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_guide) return sm_fail(SM_ERR_ARG, "%s: d_guide is NULL", me);
    if (!weights) return sm_fail(SM_ERR_ARG, "%s: weights is NULL", me);
    SM_TRY(sm_check_map_type(map_type, me, &elem));
    if (out_type != SM_MAP_I32 && out_type != SM_MAP_I16)
        return sm_fail(SM_ERR_ARG, "%s: out_type %d is neither SM_MAP_I32 nor SM_MAP_I16", me, out_type);
    out_elem = out_type == SM_MAP_I32 ? sizeof(i32) : sizeof(int16_t);
    if (!(lambda >= 0.0 && lambda <= 1048576.0)) return sm_fail(SM_ERR_ARG, "%s: lambda %g outside 0..2^20", me, lambda);
    if (iterations < 1 || iterations > WLS_MAX_T)
        return sm_fail(SM_ERR_ARG, "%s: iterations %d outside 1..%d", me, iterations, WLS_MAX_T);
    if (flags & ~SM_WLS_NO_FILL) return sm_fail(SM_ERR_ARG, "%s: flags 0x%x has bits this library does not know", me, flags);
    SM_TRY(sm_check_pairs(plan, pairs, me));
    const int W = plan->width, H = plan->height;
    const size_t n = (size_t)pairs * W * H;
    // every buffer against every other; the one overlap allowed is d_out == d_in of one type (k_wls_finish)
    const struct { const void *p; size_t bytes; const char *name; } buf[] = {
        {d_in, n * elem, "d_in"}, {d_out, n * out_elem, "d_out"}, {d_guide, n, "d_guide"}, {d_conf, n, "d_conf"},
        {d_raw, n * sizeof(double), "d_raw"}, {d_filled, (size_t)pairs * sizeof(i32), "d_filled"}};
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++) {
            if (!buf[i].p || !buf[j].p || !overlap(buf[i].p, buf[j].p, buf[i].bytes, buf[j].bytes)) continue;
            if (i == 0 && j == 1 && d_in == d_out && map_type == out_type) continue;
            return sm_fail(SM_ERR_ARG, "%s: %s overlaps %s%s", me, buf[j].name, buf[i].name,
                           i == 0 && j == 1 ? " (in place needs d_out == d_in and one type)" : "");
        }
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(sm_ws_need(plan, SM_WS_SET_WLS, st, me));
    const size_t plane = (size_t)plan->max_pairs * W * H;
    double *N = plan->d_wls, *M = N + plane, *CP = M + plane;
    const WmedTable table = wmed_table(weights);
    if (d_filled) SM_TRY(sm_lr_zero_counts(d_filled, pairs, st));
    const dim3 flat((unsigned)((n + 255) / 256));
    if (map_type == SM_MAP_I32)
        hipLaunchKernelGGL(k_wls_init<i32>, flat, dim3(256), 0, st, (const i32 *)d_in, d_conf, N, M, n);
    else
        hipLaunchKernelGGL(k_wls_init<int16_t>, flat, dim3(256), 0, st, (const int16_t *)d_in, d_conf, N, M, n);
    SM_LAUNCH_CHECK("k_wls_init");
    const dim3 rows((H + 63) / 64, 1, pairs), cols((W + 63) / 64, 1, pairs), wave(64);
    for (int t = 0; t < iterations; t++) {
        const double lam = ((1.5 * lambda) * ldexp(1.0, 2 * (iterations - 1 - t))) / (ldexp(1.0, 2 * iterations) - 1.0);
        if (W > 1) {                                // (a line of one element is returned unchanged)
            hipLaunchKernelGGL(k_wls_rows_fwd, rows, wave, 0, st, d_guide, table, lam, N, M, CP, W, H);
            hipLaunchKernelGGL(k_wls_rows_bwd, rows, wave, 0, st, N, M, CP, W, H);
            SM_LAUNCH_CHECK("k_wls_rows");
        }
        if (H > 1) {
            hipLaunchKernelGGL(k_wls_cols_fwd, cols, wave, 0, st, d_guide, table, lam, N, M, CP, W, H);
            hipLaunchKernelGGL(k_wls_cols_bwd, cols, wave, 0, st, N, M, CP, W, H);
            SM_LAUNCH_CHECK("k_wls_cols");
        }
    }
    const unsigned npx = (unsigned)W * H;
    const dim3 grid(std::min((npx + 255) / 256, (unsigned)SM_LR_BLOCKS), pairs);
    const int in_i16 = map_type == SM_MAP_I16, no_fill = (flags & SM_WLS_NO_FILL) != 0;
    if (out_type == SM_MAP_I32)
        hipLaunchKernelGGL(k_wls_finish<i32>, grid, dim3(256), 0, st, d_in, in_i16, N, M, (i32 *)d_out, d_raw, d_filled, npx,
                           no_fill);
    else
        hipLaunchKernelGGL(k_wls_finish<int16_t>, grid, dim3(256), 0, st, d_in, in_i16, N, M, (int16_t *)d_out, d_raw, d_filled,
                           npx, no_fill);
    SM_LAUNCH_CHECK("k_wls_finish");
    return SM_OK;
}
