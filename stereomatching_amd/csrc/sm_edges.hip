// sm_edges.hip -- step 1 (include/stereo_hip.h): edge detection straight into the packed ext
// image (k_edges_ext4, four pixels per lane; k_edges_ext, any width), the per-threshold decision tables behind them,
// u8 -> ext packing (sm_load_edges), and the exhaustive decision tables the tests read (sm_debug_edge_table*).
// The tables' state (tab_valid, tab_threshold, tab_ok) and pairs_loaded are written here and nowhere else.

#include "sm_internal.h"

#include <string.h>
#include <type_traits>

// ---------------------------------------------------------------------------
// step 1: edges, written directly in the hot path's packed format
// ---------------------------------------------------------------------------

// The 3-vs-3 contrast test of src/stereo.c:19-27 on integer side sums in
// units of 1/256 (brightness is k/256.0, src/image.c:9-15; the ghost halo
// 128.0 is 32768).  A three-term sum of such values is exact in double, so
// (a+b+c)/3.0 == sum/768.0 with a single rounding, and every later operation
// is one IEEE operation exactly as in the C source.  Built with
// -ffp-contract=off; tests/test_hip_gpu.py (test_edge_decision_exhaustive) checks
// all 766*766 in-image sum pairs against the host's arithmetic.
__device__ __forceinline__ bool contrast_test(int sa, int sb, double threshold)
{
    const double ma = (double)sa / 768.0;
    const double mb = (double)sb / 768.0;
    const double overall = (ma + mb) / 2.0;
    double limit = threshold * overall;
    limit = limit > 0.0 ? limit : 0.0;
    limit = limit < 1.0 ? limit : 1.0;
    return fabs(ma - mb) > limit;
}

__device__ __forceinline__ int pos_mod(int v, int m)
{
    int r = v % m;
    return r < 0 ? r + m : r;
}

// edge value of image pixel (x, y), 0 <= x < w, 0 <= y < h
__device__ __forceinline__ u32 edge_at(const u8 *__restrict__ gray, int w, int h, int x, int y,
                                       double threshold, bool ghost)
{
    int v[3][3];
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            int xx = x + dx, yy = y + dy;
            int val;
            if (ghost) {
                const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
                val = in ? gray[(size_t)yy * w + xx] : 32768;
            } else {
                xx = xx < 0 ? w - 1 : (xx >= w ? 0 : xx);
                yy = yy < 0 ? h - 1 : (yy >= h ? 0 : yy);
                val = gray[(size_t)yy * w + xx];
            }
            v[dy + 1][dx + 1] = val;
        }
    }
    // v[row][col]: row 0 = y-1, col 0 = x-1
    // left | right                       src/stereo.c:16-28
    if (contrast_test(v[0][0] + v[1][0] + v[2][0], v[0][2] + v[1][2] + v[2][2], threshold)) return 1;
    // top | bottom                       src/stereo.c:30-42
    if (contrast_test(v[0][0] + v[0][1] + v[0][2], v[2][0] + v[2][1] + v[2][2], threshold)) return 1;
    // up-left | down-right               src/stereo.c:44-56
    if (contrast_test(v[0][0] + v[0][1] + v[1][0], v[1][2] + v[2][1] + v[2][2], threshold)) return 1;
    // down-left | up-right               src/stereo.c:58-70
    if (contrast_test(v[2][0] + v[2][1] + v[1][0], v[0][1] + v[0][2] + v[1][2], threshold)) return 1;
    return 0;
}

__global__ void k_edge_table(double threshold, u8 *__restrict__ table)
{
    const int sb = blockIdx.x * blockDim.x + threadIdx.x, sa = blockIdx.y;
    if (sb < 766) table[sa * 766 + sb] = contrast_test(sa, sb, threshold);
}

// Per-threshold decision tables.  For a fixed left sum sa the exact test is
// true for right sums sb <= lo(sa) and sb >= hi(sa) and false in between: with
// sb moving away from sa, |ma - mb| grows by 1/768 per unit and the limit
// threshold*(ma+mb)/2 by at most 1/1536, so the difference is monotone by a
// margin of ~1e-3, far above the rounding of the double operations.  The
// tables are BUILT with the exact double test (one workgroup per sa evaluates
// all 766 sb) and the threshold form is VERIFIED while building: if any row is
// not "true prefix, false middle, true suffix", bad_flag is raised and the
// edge kernel keeps using the double arithmetic.  The edge kernel then needs
// two integer compares per orientation instead of two double divisions.
__global__ __launch_bounds__(256) void k_edge_thresholds(double threshold, u32 *__restrict__ tab,
                                                         i32 *__restrict__ bad_flag)
{
    __shared__ int lo, hi, n_lo, n_hi;
    const int sa = blockIdx.x;
    if (threadIdx.x == 0) { lo = -1; hi = 766; n_lo = 0; n_hi = 0; }
    __syncthreads();
    for (int sb = threadIdx.x; sb < 766; sb += blockDim.x) {
        if (contrast_test(sa, sb, threshold)) {
            if (sb <= sa) { atomicMax(&lo, sb); atomicAdd(&n_lo, 1); }
            if (sb >= sa) { atomicMin(&hi, sb); atomicAdd(&n_hi, 1); }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tab[sa] = (u32)(lo & 0xffff) | ((u32)hi << 16);   // lo = -1 -> 0xffff (never <=)
        if (n_lo != lo + 1 || n_hi != 766 - hi) atomicOr(bad_flag, 1);
    }
}

// f32 prefilter in front of the tables.  In exact arithmetic the test is
//     E = |sa - sb| - theta * (sa + sb) > 0,   theta = threshold / 2
// (the clamp to [0,1] never binds for in-image sums).  The sums are integers
// below 2^11, exact in f32; with T = (float)theta,
//     F = fma(sa + sb, -T, |sa - sb|)                        (one rounding)
// differs from E by at most 1530 * |T - theta| <= 1530 * 2^-26 < 2.3e-5 plus the
// fma rounding, which is <= 2^-25 whenever |F| < 1.  So |F| > 2^-12 (2.4e-4)
// leaves a real margin > 2e-4 sum units -- a relative margin > 1e-7 on
// quantities the double evaluation gets right to ~1e-15: the sign of F IS the
// double decision.  Only |F| <= 2^-12 (the few sum pairs next to the boundary)
// consults the table.  Same function in the edge kernels and in the exhaustive
// debug table, so the test covers what runs.  Three full-rate VALU operations
// per orientation (the abs and the negation are source modifiers).
#define SM_EDGE_MARGIN 0.000244140625f
__device__ __forceinline__ float edge_delta(float sa, float sb, float neg_t)
{
    return __builtin_fmaf(sa + sb, neg_t, __builtin_fabsf(sa - sb));
}
__device__ __forceinline__ bool edge_from_table(const u32 *tab, int sa, int sb)
{
    const u32 lh = tab[sa];
    return sb <= (int)(short)(lh & 0xffff) || sb >= (int)(lh >> 16);
}

__global__ void k_edge_table_fast(const u32 *__restrict__ tab, float neg_t, u8 *__restrict__ table)
{
    const int sb = blockIdx.x * blockDim.x + threadIdx.x, sa = blockIdx.y;
    if (sb >= 766) return;
    const float delta = edge_delta((float)sa, (float)sb, neg_t);
    table[sa * 766 + sb] = delta > SM_EDGE_MARGIN ? 1 : delta < -SM_EDGE_MARGIN ? 0
                                                      : edge_from_table(tab, sa, sb);
}

#define SM_EDGE_ROWS 32   // ext rows one wave walks down

// byte B of a dword as f32 (v_cvt_f32_ubyteB)
template <int B> __device__ __forceinline__ float cvt_ubyte(u32 q)
{
    float f;
    if (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(q));
    if (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(q));
    if (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(q));
    if (B == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(q));
    return f;
}

// One pixel's decision from its 8 orientation sums (f32, exact integers).
// sa/sb order: left|right, top|bottom, up-left|down-right, down-left|up-right
// (src/stereo.c:16-70).  `exact` (ghost pixels on or outside the image border,
// whose sums contain the 128.0 halo and are outside the tables; or no usable
// tables at all) takes the double arithmetic of the reference.
// `known_edge`: a ghost-mode pixel ON the image border of an image at least 2 x 2.  One of
// its axis-aligned tests has three halo pixels (128.0 each) on one side and only in-image
// pixels (< 1.0 each) on the other -- or, at a corner, two halo pixels more on one side than
// on the other -- so the side means differ by more than 40 while the limit is clamped to
// [0, 1] (src/stereo-ghost.c:18-30): it is an edge for every threshold, and no arithmetic
// is spent on it (the double path it used to take made ghost-mode edges 4x slower).
template <bool TABLES>
__device__ __forceinline__ u32 edge_decide(const float (&sa)[4], const float (&sb)[4],
                                           const u32 *__restrict__ tab, double threshold,
                                           float neg_t, bool exact, bool known_edge = false)
{
    u32 e;
    if (TABLES) {
        float dl[4];
#pragma unroll
        for (int o = 0; o < 4; o++) dl[o] = edge_delta(sa[o], sb[o], neg_t);
        const float dmax = fmaxf(fmaxf(dl[0], dl[1]), fmaxf(dl[2], dl[3]));
        e = __float_as_uint(SM_EDGE_MARGIN - dmax) >> 31;                 // dmax > margin
        // rare: the deciding sum pair is next to the boundary -> ask the table
        // (never with halo sums: they are not table indices)
        if (!exact && !known_edge && __builtin_fabsf(dmax) <= SM_EDGE_MARGIN) {
#pragma unroll
            for (int o = 0; o < 4; o++)
                if (dl[o] >= -SM_EDGE_MARGIN)
                    e |= edge_from_table(tab, (int)sa[o], (int)sb[o]) ? 1u : 0u;
        }
    }
    if (!TABLES || exact) {
        e = 0;
#pragma unroll
        for (int o = 0; o < 4; o++)
            e |= contrast_test((int)sa[o], (int)sb[o], threshold) ? 1u : 0u;
    }
    return known_edge ? 1u : e;
}

// Edge detection straight into the packed ext image.  No LDS, no barrier: a
// wave owns a strip of 64 ext pixels x SM_EDGE_ROWS ext rows and walks down it;
// each lane keeps the 3 x 3 gray neighbourhood of its pixel in registers and
// loads three bytes (x-1, x, x+1) of the next row per step.  The wave's 64
// decisions become two ext words via ballot.  Border rule at load time: wrapped
// coordinates (toroidal) or the 128.0 halo, 32768 in units of 1/256 (ghost).
// This is the any-width kernel; widths that are a multiple of 4 take
// k_edges_ext4 below.
template <bool GHOST, bool TABLES>
__global__ __launch_bounds__(256) void k_edges_ext(const u8 *__restrict__ src_l,
                                                   const u8 *__restrict__ src_r,
                                                   u8 *__restrict__ edges_l,
                                                   u8 *__restrict__ edges_r,
                                                   u32 *__restrict__ ext,
                                                   const u32 *__restrict__ tab,
                                                   const MatchGeom g, double threshold, float neg_t)
{
    const int tid = threadIdx.x;
    const int xe = blockIdx.x * 256 + tid;
    const int ye0 = blockIdx.y * SM_EDGE_ROWS;
    const int pair = blockIdx.z >> 1, side = blockIdx.z & 1;
    const size_t img = (size_t)pair * g.w * g.h;
    const u8 *src = (side ? src_r : src_l) + img;
    u8 *edges = side ? edges_r : edges_l;

    const int x = xe - g.pad_l;
    const u32 in_x = (xe < g.ext_words * 32 && (!GHOST || (x >= 0 && x < g.w))) ? 1u : 0u;
    const bool store_x = x >= 0 && x < g.w && edges != nullptr;
    const bool inner_x = x > 0 && x < g.w - 1;             // ghost: no halo in the 3 columns
    u32 *ext_img = ext + (size_t)blockIdx.z * g.ext_rows * g.ext_words;
    const int wd = xe >> 5;

    // source columns of x-1, x, x+1
    int xc[3];
    bool vx[3];
    if (GHOST) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int xx = x - 1 + k;
            vx[k] = xx >= 0 && xx < g.w;
            xc[k] = vx[k] ? xx : 0;
        }
    } else {
        xc[1] = pos_mod(x, g.w);
        xc[0] = xc[1] == 0 ? g.w - 1 : xc[1] - 1;
        xc[2] = xc[1] + 1 == g.w ? 0 : xc[1] + 1;
        vx[0] = vx[1] = vx[2] = true;
    }

    // rows: image row of ext row ye is ye - half; the walk starts one above
    int y_img = ye0 - g.half - 1;
    int ys = GHOST ? y_img : pos_mod(y_img, g.h);       // source row (toroidal: wrapped)
    auto load_row = [&](float (&o)[3]) {
        const bool vy = !GHOST || (y_img >= 0 && y_img < g.h);
        const u8 *row = src + (size_t)(vy ? ys : 0) * g.w;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = (float)row[xc[k]];
            o[k] = (vy && vx[k]) ? v : 32768.0f;
        }
        y_img++;
        ys = GHOST ? y_img : (ys + 1 == g.h ? 0 : ys + 1);
    };

    float v[3][3];          // v[row][col]: row 0 = y-1, col 0 = x-1
    load_row(v[0]);
    load_row(v[1]);
    const int rows = min(SM_EDGE_ROWS, g.ext_rows - ye0);
    for (int rr = 0; rr < rows; rr++) {
        load_row(v[2]);
        const int ye = ye0 + rr;
        const int y = ye - g.half;
        const bool in_y = y >= 0 && y < g.h;         // uniform
        const float sa[4] = {v[0][0] + v[1][0] + v[2][0],      // left      src/stereo.c:16-28
                             v[0][0] + v[0][1] + v[0][2],      // top       src/stereo.c:30-42
                             v[0][0] + v[0][1] + v[1][0],      // up-left   src/stereo.c:44-56
                             v[2][0] + v[2][1] + v[1][0]};     // down-left src/stereo.c:58-70
        const float sb[4] = {v[0][2] + v[1][2] + v[2][2],      // right
                             v[2][0] + v[2][1] + v[2][2],      // bottom
                             v[1][2] + v[2][1] + v[2][2],      // down-right
                             v[0][1] + v[0][2] + v[1][2]};     // up-right
        const bool on_border = GHOST && !(inner_x && y > 0 && y < g.h - 1);
        const bool big = g.w >= 2 && g.h >= 2;         // uniform
        const bool exact = on_border && !(TABLES && big);
        const u32 e = edge_decide<TABLES>(sa, sb, tab, threshold, neg_t, exact, on_border && TABLES && big);
        const u32 val = e & in_x & ((!GHOST || in_y) ? 1u : 0u);
        if (store_x && in_y) edges[img + (size_t)y * g.w + x] = (u8)val;
        const unsigned long long bal = __ballot(val != 0);
        if ((tid & 63) == 0) {
            u32 *row = ext_img + (size_t)ye * g.ext_words;
            if (wd < g.ext_words) row[wd] = (u32)bal;
            if (wd + 1 < g.ext_words) row[wd + 1] = (u32)(bal >> 32);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) { v[0][k] = v[1][k]; v[1][k] = v[2][k]; }
    }
}

// Same decision, FOUR pixels per lane (images whose width is a multiple of 4).
// Per row a lane loads ONE aligned dword (its 4 gray values); the pixels left
// and right of the quad are bytes of the neighbouring lanes' dwords, fetched
// with DPP wave shifts -- only lane 0 / lane 63 of a wave need a real byte load
// (one instruction serves both).  A wave's whole strip is SM_EDGE4_ROWS + 2
// rows: ALL its loads are issued before the first decision (the row loop is
// unrolled over a compile-time row count), so a wave pays the HBM latency once
// instead of once per row -- the row-at-a-time version of this kernel spent half
// its wave-cycles waiting.  Sums are shared: per row the 5 pair sums and 4 triple
// sums of horizontally adjacent pixels are formed once and carried down (the
// bottom sums of row y are the top sums of row y+2); column sums serve as `left`
// of one pixel and `right` of another.  A lane's 4 decisions form a nibble; 8
// adjacent lanes OR their nibbles together (DPP) into one ext word.
#define SM_EDGE4_ROWS 4   // ext rows of a wave's strip (8: profiles/r05/ab_edge_strips_rejected.txt)
template <bool GHOST, bool TABLES, bool STACKED = false>
__global__ __launch_bounds__(256) void k_edges_ext4(const u8 *__restrict__ src_l,
                                                    const u8 *__restrict__ src_r,
                                                    u8 *__restrict__ edges_l,
                                                    u8 *__restrict__ edges_r,
                                                    u32 *__restrict__ ext,
                                                    const u32 *__restrict__ tab,
                                                    const MatchGeom g, double threshold, float neg_t)
{
    constexpr int R = SM_EDGE4_ROWS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // The workgroup's four waves lie side by side in one strip or (STACKED) take four strips
    // below each other, 256 ext pixels wide: the host picks the second where the round-up
    // of a 1024-pixel workgroup along x would leave much of the launch idle (a 1080p ext row
    // is 560 lanes: 9 waves instead of 12; 8 x 1080p: 40.8 -> 34.0 us; C5: 29.5 -> 26.1) and
    // the first where a row is whole workgroups anyway (4K toroidal: 17.0 vs 18.1 us stacked).
    // first of this lane's 4 ext pixels, first ext row of the wave's strip
    const int xe = STACKED ? (blockIdx.x * 64 + lane) * 4 : (blockIdx.x * 256 + tid) * 4;
    const int ye0 = STACKED ? (blockIdx.y * 4 + (tid >> 6)) * R : blockIdx.y * R;
    if (STACKED && ye0 >= g.ext_rows) return;             // the round-up of the strips (wave-uniform)
    // columns no valid output pixel can reach (the match kernel's tile round-up; for the left image
    // also the shift range): left as they are (wave-uniform).  Zero since the plan was created, or -- after an
    // sm_load_edges, whose k_pack_ext writes every ext column -- stale content of that call: either way no stored
    // output pixel reads them (tests: sm_load_edges, then sm_find_edges and the match launch on one plan)
    if (((xe - 4 * lane) >> 5) >= ((blockIdx.z & 1) ? g.edge_words_r : g.edge_words_l)) return;
    const int pair = blockIdx.z >> 1, side = blockIdx.z & 1;
    const size_t img = (size_t)pair * g.w * g.h;
    const u8 *src = (side ? src_r : src_l) + img;
    u8 *edges = side ? edges_r : edges_l;

    const int x = xe - g.pad_l;                            // multiple of 4
    const bool in_ext = xe < g.ext_words * 32;
    const bool quad_in = x >= 0 && x < g.w;                // all 4 inside (w % 4 == 0)
    const bool inner_x = x > 0 && x + 4 < g.w;             // ghost: no halo in the 6 columns
    u32 *ext_img = ext + (size_t)blockIdx.z * g.ext_rows * g.ext_words;
    const int wd = xe >> 5;

    // Ghost mode: a wave whose strip, with its one-pixel ring of neighbours, lies strictly inside the
    // image (x in [1, w - 2], y in [1, h - 2]) meets no halo, no border pixel and no round-up: it runs
    // the body without a single validity select (`SEL` false) -- at 4K that is 97 % of the waves; the
    // others keep the selects.  Toroidal mode has no selects to begin with.
    auto body = [&](auto sel_tag) {
        constexpr bool SEL = decltype(sel_tag)::value;
        // source columns: the aligned quad; the single pixel left (lane 0) or right
        // (lane 63) of the wave's span -- the other lanes' value of `xn` is unused
        int xq, xn;
        bool vq, vl, vr;
        if (GHOST && !SEL) {
            vq = vl = vr = true;
            xq = x;
            xn = lane == 63 ? x + 4 : x - 1;
        } else if (GHOST) {
            vq = quad_in; vl = x - 1 >= 0 && x - 1 < g.w; vr = x + 4 >= 0 && x + 4 < g.w;
            xq = vq ? x : 0;
            xn = lane == 63 ? (vr ? x + 4 : 0) : (vl ? x - 1 : 0);
        } else {
            // x is in [-pad_l, ext width - pad_l): one conditional add or subtract wraps it
            // whenever the image is at least as wide as either pad (the usual case);
            // the division is the fallback for images narrower than their padding
            const int over = g.ext_words * 32 - g.pad_l - g.w;     // uniform: columns right of the image
            if (g.w >= g.pad_l && g.w >= over) xq = x < 0 ? x + g.w : (x >= g.w ? x - g.w : x);
            else                               xq = pos_mod(x, g.w);
            // lanes of the grid's round-up beyond the ext image load nothing meaningful, but
            // they do load: keep their addresses inside the row (one wrap is not enough there)
            if (!in_ext) xq = 0;
            xn = lane == 63 ? (xq + 4 == g.w ? 0 : xq + 4) : (xq == 0 ? g.w - 1 : xq - 1);
            vq = vl = vr = true;
        }

        // all loads of the strip: rows ye0-half-1 ... ye0-half+R (border rule on the row)
        u32 q4[R + 2], nb[R + 2];
        bool vy[R + 2];
        {
            int y_img = ye0 - g.half - 1;
            // wrapped source row of the strip's first row: y_img >= -half - 1 >= -h always; one
            // conditional add or subtract covers up to 2h, the division (a few dozen scalar
            // instructions per wave, on the CU's one scalar unit: 6 % of this kernel's time) is
            // left for the round-up rows of very small images
            int ys = y_img;
            if (!GHOST) ys = y_img < 0 ? y_img + g.h : (y_img < g.h ? y_img : (y_img < 2 * g.h ? y_img - g.h : pos_mod(y_img, g.h)));
    #pragma unroll
            for (int k = 0; k < R + 2; k++) {
                vy[k] = !SEL || (y_img >= 0 && y_img < g.h);
                const u8 *row = src + (size_t)(vy[k] ? ys : 0) * g.w;
                q4[k] = *reinterpret_cast<const u32 *>(row + xq);
                nb[k] = row[xn];
                y_img++;
                ys = GHOST ? y_img : (ys + 1 == g.h ? 0 : ys + 1);
            }
        }
        // gray values of a row as f32 (col 0 = x-1 ... col 5 = x+4), its pair and triple sums
        auto unpack_row = [&](int k, float (&o)[6], float (&p)[5], float (&s3)[4]) {
            const u32 q = q4[k];
            // lane i-1's / lane i+1's dword (wave_shr:1 / wave_shl:1)
            const u32 from_l = (u32)__builtin_amdgcn_update_dpp(0, (int)q, 0x138, 0xf, 0xf, false);
            const u32 from_r = (u32)__builtin_amdgcn_update_dpp(0, (int)q, 0x130, 0xf, 0xf, false);
            const u32 lq = lane == 0 ? nb[k] << 24 : from_l;
            const u32 rq = lane == 63 ? nb[k] : from_r;
            // v_cvt_f32_ubyteN: byte -> f32 in one instruction, and opaque to the
            // optimiser (plain casts get their f32 sums folded back into integer adds
            // plus one conversion per SUM, which is more work)
            const float g0 = cvt_ubyte<0>(q), g1 = cvt_ubyte<1>(q),
                        g2 = cvt_ubyte<2>(q), g3 = cvt_ubyte<3>(q);
            const bool okq = vy[k] && vq;
            o[0] = (vy[k] && vl) ? cvt_ubyte<3>(lq) : 32768.0f;
            o[1] = okq ? g0 : 32768.0f;
            o[2] = okq ? g1 : 32768.0f;
            o[3] = okq ? g2 : 32768.0f;
            o[4] = okq ? g3 : 32768.0f;
            o[5] = (vy[k] && vr) ? cvt_ubyte<0>(rq) : 32768.0f;
    #pragma unroll
            for (int c = 0; c < 5; c++) p[c] = o[c] + o[c + 1];
    #pragma unroll
            for (int c = 0; c < 4; c++) s3[c] = p[c] + o[c + 2];
        };

        float v[3][6], p[3][5], s3[3][4];      // [row][col]: row 0 = y-1
        unpack_row(0, v[0], p[0], s3[0]);
        unpack_row(1, v[1], p[1], s3[1]);
    #pragma unroll
        for (int rr = 0; rr < R; rr++) {
            unpack_row(rr + 2, v[2], p[2], s3[2]);
            const int ye = ye0 + rr;
            const int y = ye - g.half;
            const bool in_y = y >= 0 && y < g.h;         // uniform
            // ghost: pixels on the image border are edges by construction (edge_decide); only
            // images narrower or lower than 2 keep the double path for them
            const bool big = g.w >= 2 && g.h >= 2;                       // uniform
            const bool row_border = SEL && (y <= 0 || y >= g.h - 1);     // uniform
            const bool exact = SEL && !(TABLES && big) && !(inner_x && y > 0 && y < g.h - 1);
            float col[6];
    #pragma unroll
            for (int k = 0; k < 6; k++) col[k] = v[0][k] + v[1][k] + v[2][k];
            u32 nib = 0;
    #pragma unroll
            for (int q = 0; q < 4; q++) {
                // 3x3 neighbourhood of pixel q: columns q, q+1, q+2 of v
                const float sa[4] = {col[q],                       // left      src/stereo.c:16-28
                                     s3[0][q],                     // top       src/stereo.c:30-42
                                     p[0][q] + v[1][q],            // up-left   src/stereo.c:44-56
                                     p[2][q] + v[1][q]};           // down-left src/stereo.c:58-70
                const float sb[4] = {col[q + 2],                   // right
                                     s3[2][q],                     // bottom
                                     p[2][q + 1] + v[1][q + 2],    // down-right
                                     p[0][q + 1] + v[1][q + 2]};   // up-right
                const bool known = SEL && TABLES && big && (row_border || x + q <= 0 || x + q >= g.w - 1);
                nib |= edge_decide<TABLES>(sa, sb, tab, threshold, neg_t, exact, known) << q;
            }
            if (GHOST ? (SEL && !(in_ext && quad_in && in_y)) : !in_ext) nib = 0;
            const bool row_ok = (GHOST && !SEL) || ye < g.ext_rows;   // uniform; the last strip may be short
            if (edges != nullptr && ((GHOST && !SEL) || (quad_in && in_y && row_ok))) {
                // u8 {0,1} per pixel: bit q of the nibble -> byte q
                const u32 bytes = __umul24(nib, 0x204081u) & 0x01010101u;
                *reinterpret_cast<u32 *>(edges + img + (size_t)y * g.w + x) = bytes;
            }
            // 8 lanes x 4 bits -> one ext word, OR-reduced within each group of 8 lanes
            u32 wv = nib << (4 * (lane & 7));
            wv |= (u32)__builtin_amdgcn_update_dpp(0, (int)wv, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
            wv |= (u32)__builtin_amdgcn_update_dpp(0, (int)wv, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
            wv |= (u32)__builtin_amdgcn_update_dpp(0, (int)wv, 0x141, 0xf, 0xf, true);   // row_half_mirror
            if ((lane & 7) == 0 && wd < g.ext_words && row_ok) ext_img[(size_t)ye * g.ext_words + wd] = wv;
    #pragma unroll
            for (int k = 0; k < 6; k++) { v[0][k] = v[1][k]; v[1][k] = v[2][k]; }
    #pragma unroll
            for (int k = 0; k < 5; k++) { p[0][k] = p[1][k]; p[1][k] = p[2][k]; }
    #pragma unroll
            for (int k = 0; k < 4; k++) { s3[0][k] = s3[1][k]; s3[1][k] = s3[2][k]; }
        }
    };
    if (GHOST) {
        const int x0 = xe - 4 * lane - g.pad_l, y0 = ye0 - g.half;        // the wave's first pixel / row
        const bool inside = x0 >= 1 && x0 + 256 <= g.w - 1 && y0 >= 1 && y0 + R - 1 <= g.h - 2 &&
                            ye0 + R <= g.ext_rows && g.w >= 2 && g.h >= 2;
        if (inside) body(std::false_type{});
        else        body(std::true_type{});
    } else {
        body(std::false_type{});
    }
}

// u8 {0,1} edge image -> packed ext image (the sm_load_edges entry).  One lane
// per ext pixel; a wave's 64 values become two ext words via ballot.
__global__ __launch_bounds__(256) void k_pack_ext(const u8 *__restrict__ src_l,
                                                  const u8 *__restrict__ src_r,
                                                  u32 *__restrict__ ext, const MatchGeom g, int ghost)
{
    const int xe = blockIdx.x * blockDim.x + threadIdx.x;
    const int ye = blockIdx.y;
    const int pair = blockIdx.z >> 1, side = blockIdx.z & 1;
    const u8 *src = (side ? src_r : src_l) + (size_t)pair * g.w * g.h;
    const int x = xe - g.pad_l, y = ye - g.half;
    const bool inside = x >= 0 && x < g.w && y >= 0 && y < g.h;
    u32 val = 0;
    if (xe < g.ext_words * 32 && (inside || !ghost)) {
        const int xs = inside ? x : pos_mod(x, g.w);
        const int ys = inside ? y : pos_mod(y, g.h);
        val = src[(size_t)ys * g.w + xs] != 0;
    }
    const unsigned long long bal = __ballot(val != 0);
    if ((threadIdx.x & 63) == 0) {
        u32 *row = ext + ((size_t)blockIdx.z * g.ext_rows + ye) * g.ext_words;
        const int wd = xe >> 5;
        if (wd < g.ext_words) row[wd] = (u32)bal;
        if (wd + 1 < g.ext_words) row[wd + 1] = (u32)(bal >> 32);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

void sm_edges_resolve_kernels(bool ghost)
{
    hipFuncAttributes fa;
    for (const void *f : {(const void *)k_edge_thresholds, (const void *)k_pack_ext,
                          ghost ? (const void *)k_edges_ext4<true, true> : (const void *)k_edges_ext4<false, true>,
                          ghost ? (const void *)k_edges_ext4<true, true, true> : (const void *)k_edges_ext4<false, true, true>,
                          ghost ? (const void *)k_edges_ext<true, true> : (const void *)k_edges_ext<false, true>})
        (void)hipFuncGetAttributes(&fa, f);
}

int sm_edges_rows_per_wave(const sm_plan *plan) { return plan->g.w % 4 == 0 ? SM_EDGE4_ROWS : SM_EDGE_ROWS; }

static int pack_ext(sm_plan *plan, const u8 *l, const u8 *r, int pairs, hipStream_t st)
{
    const MatchGeom &g = plan->g;
    const dim3 grid((g.ext_words * 32 + 255) / 256, g.ext_rows, pairs * 2), block(256);
    hipLaunchKernelGGL(k_pack_ext, grid, block, 0, st, l, r, plan->d_ext, g,
                       plan->border == SM_GHOST ? 1 : 0);
    SM_LAUNCH_CHECK("k_pack_ext");
    plan->pairs_loaded = pairs;
    return SM_OK;
}

static float edge_neg_t(double threshold)
{
    return -(float)(threshold * 0.5);
}

bool sm_edge_tables_prepared(const sm_plan *plan, double threshold)
{
    return plan->tab_valid && memcmp(&plan->tab_threshold, &threshold, sizeof threshold) == 0;
}

int sm_check_tables_prepared(const sm_plan *plan, double threshold, const char *me)
{
    if (!sm_edge_tables_prepared(plan, threshold))
        return sm_fail(SM_ERR_ARG, "%s: the decision tables of threshold %g are not prepared and the stream is capturing: "
                       "call sm_plan_prepare_threshold(plan, threshold, stream) before the capture begins", me, threshold);
    return SM_OK;
}

// decision tables depend on the threshold only: rebuilt when it changes
static int ensure_edge_tables(sm_plan *plan, double threshold, hipStream_t st)
{
    if (sm_edge_tables_prepared(plan, threshold)) return SM_OK;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "the decision tables of threshold %g are not prepared and the stream is capturing: their "
                       "set-up reads a verdict back to the host, which a graph cannot hold -- call "
                       "sm_plan_prepare_threshold(plan, threshold, stream) before the capture begins", threshold);
    SM_HIP(hipMemsetAsync(&plan->d_flags[2], 0, sizeof(i32), st));
    hipLaunchKernelGGL(k_edge_thresholds, dim3(766), dim3(256), 0, st, threshold,
                       plan->d_edge_tab, &plan->d_flags[2]);
    SM_LAUNCH_CHECK("k_edge_thresholds");
    // read the verdict back once per new threshold (not in the steady state): it
    // selects the kernel instantiation
    i32 f[4];
    SM_TRY(sm_read_flags(plan, st, 0, f));
    plan->tab_ok = f[2] == 0;
    plan->tab_threshold = threshold;
    plan->tab_valid = 1;
    return SM_OK;
}

extern "C" int sm_debug_edge_table_fast(sm_plan *plan, double threshold, uint8_t *d_table,
                                        int *not_threshold_form, void *stream)
{
    if (!plan || !d_table || !not_threshold_form)
        return sm_fail(SM_ERR_ARG, "sm_debug_edge_table_fast: NULL argument");
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(ensure_edge_tables(plan, threshold, st));
    hipLaunchKernelGGL(k_edge_table_fast, dim3(3, 766), dim3(256), 0, st, plan->d_edge_tab,
                       edge_neg_t(threshold), d_table);
    SM_LAUNCH_CHECK("k_edge_table_fast");
    i32 f[4];
    SM_TRY(sm_read_flags(plan, st, 0, f));
    *not_threshold_form = f[2];
    return SM_OK;
}

extern "C" int sm_plan_prepare_threshold(sm_plan *plan, double threshold, void *stream)
{
    if (!plan) return sm_fail(SM_ERR_ARG, "sm_plan_prepare_threshold: plan is NULL");
    SM_TRY(sm_check_threshold(threshold, "sm_plan_prepare_threshold"));
    SM_TRY(sm_use_device(plan->device));
    return ensure_edge_tables(plan, threshold, (hipStream_t)stream);
}

extern "C" int sm_find_edges(sm_plan *plan, const uint8_t *d_gray_left,
                             const uint8_t *d_gray_right, double threshold, int pairs,
                             uint8_t *d_edges_left, uint8_t *d_edges_right, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_find_edges"));
    if (!d_gray_left || !d_gray_right)
        return sm_fail(SM_ERR_ARG, "sm_find_edges: input image pointer is NULL");
    SM_TRY(sm_check_threshold(threshold, "sm_find_edges"));
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    SM_TRY(ensure_edge_tables(plan, threshold, st));
    const MatchGeom &g = plan->g;
    const dim3 grid((g.edge_words_r * 32 + 255) / 256, (g.ext_rows + SM_EDGE_ROWS - 1) / SM_EDGE_ROWS,
                    pairs * 2), block(256);
    const bool ghost = plan->border == SM_GHOST;
    // the 4-pixels-per-lane kernel moves dwords: rows (w % 4 == 0) and base pointers
    // must be 4-byte aligned, else the any-width kernel takes over
    const bool aligned4 = (((uintptr_t)d_gray_left | (uintptr_t)d_gray_right |
                            (uintptr_t)d_edges_left | (uintptr_t)d_edges_right) & 3) == 0;
    if (g.w % 4 == 0 && aligned4 && plan->opt.edge_kernel != 1) {
        const int strips = (g.ext_rows + SM_EDGE4_ROWS - 1) / SM_EDGE4_ROWS;
        const int lanes = g.edge_words_r * 8;       // (the left image's waves beyond its own need leave at once)
        // waves side by side, unless that rounds the row up by more than 3 % (see the kernel)
        const bool stacked = (lanes + 255) / 256 * 256 > lanes + lanes / 32;
        const dim3 grid4 = stacked ? dim3((lanes + 63) / 64, (strips + 3) / 4, pairs * 2)
                                   : dim3((lanes + 255) / 256, strips, pairs * 2);
#define SM_EDGES_GO(G, T)                                                                      \
    do {                                                                                       \
        if (stacked)                                                                           \
            hipLaunchKernelGGL((k_edges_ext4<G, T, true>), grid4, block, 0, st, d_gray_left, d_gray_right, \
                               d_edges_left, d_edges_right, plan->d_ext, plan->d_edge_tab, g, threshold,   \
                               edge_neg_t(threshold));                                         \
        else                                                                                   \
            hipLaunchKernelGGL((k_edges_ext4<G, T, false>), grid4, block, 0, st, d_gray_left, d_gray_right, \
                               d_edges_left, d_edges_right, plan->d_ext, plan->d_edge_tab, g, threshold,   \
                               edge_neg_t(threshold));                                         \
    } while (0)
        if (plan->tab_ok) { if (ghost) SM_EDGES_GO(true, true); else SM_EDGES_GO(false, true); }
        else              { if (ghost) SM_EDGES_GO(true, false); else SM_EDGES_GO(false, false); }
#undef SM_EDGES_GO
    } else {
#define SM_EDGES_GO(G, T)                                                                      \
    hipLaunchKernelGGL((k_edges_ext<G, T>), grid, block, 0, st, d_gray_left, d_gray_right,       \
                       d_edges_left, d_edges_right, plan->d_ext, plan->d_edge_tab, g, threshold, \
                       edge_neg_t(threshold))
        if (plan->tab_ok) { if (ghost) SM_EDGES_GO(true, true); else SM_EDGES_GO(false, true); }
        else              { if (ghost) SM_EDGES_GO(true, false); else SM_EDGES_GO(false, false); }
#undef SM_EDGES_GO
    }
    SM_LAUNCH_CHECK("k_edges_ext");
    plan->pairs_loaded = pairs;
    return SM_OK;
}

extern "C" int sm_load_edges(sm_plan *plan, const uint8_t *d_edges_left,
                             const uint8_t *d_edges_right, int pairs, void *stream)
{
    SM_TRY(sm_check_pairs(plan, pairs, "sm_load_edges"));
    if (!d_edges_left || !d_edges_right)
        return sm_fail(SM_ERR_ARG, "sm_load_edges: edge image pointer is NULL");
    SM_TRY(sm_use_device(plan->device));
    return pack_ext(plan, d_edges_left, d_edges_right, pairs, (hipStream_t)stream);
}

extern "C" int sm_debug_edge_table(int device, double threshold, uint8_t *d_table, void *stream)
{
    if (!d_table) return sm_fail(SM_ERR_ARG, "sm_debug_edge_table: d_table is NULL");
    SM_TRY(sm_use_device(device));
    hipLaunchKernelGGL(k_edge_table, dim3(3, 766), dim3(256), 0, (hipStream_t)stream, threshold,
                       d_table);
    SM_LAUNCH_CHECK("k_edge_table");
    return SM_OK;
}
