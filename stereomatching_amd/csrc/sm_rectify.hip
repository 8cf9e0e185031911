// sm_rectify.hip -- stereo rectification (include/stereo_hip.h "rectification").
//
//   k_rectify        the remap: every destination pixel reads the raw image where a fixed-point map says, bilinear or
//                    nearest, with a validity bit.  Integer arithmetic throughout.
//   k_rmap_build     the map of a calibration (Brown-Conrady distortion, rectifying rotation, new projection), IEEE
//                    double, one operation at a time in the order tests/rectify_reference.py fixes (this unit is
//                    compiled with -ffp-contract=off, as every file of the library is)
// (k_valid_mask, which carries the validity to a disparity map, is a post-filter: sm_filter.hip)
//
// The remap is a stream (map in, pixels out) around a gather (the raw image).  Per destination pixel it moves 8 (ABS32)
// or 4 (REL16) map bytes, one output byte, one validity byte if asked, and about one source byte that a smooth map keeps
// local: the taps of neighbouring pixels share cache lines, so the gather is served by the vector cache and L2 and
// is not staged in LDS.  A lane owns four consecutive destination pixels of a row (V = 4: W % 4 == 0, 16-byte
// aligned maps, dword aligned outputs): its map entries arrive as one (REL16) or two (ABS32) 16-byte loads and its
// pixels leave as one dword store per output.  Other widths and alignments take one pixel per lane (V = 1).  A lane
// walks the pairs of the batch itself: both sides' maps are shared by all pairs and are read once per call.
//
// Every tap is loaded from a clamped, always legal position and replaced by `border` afterwards where the position
// was outside: sixteen independent byte loads per lane and pair, no divergent branch.

#include "sm_internal.h"

#define SM_RECT_FRAC 5      // SM_RMAP_FRAC_BITS
#define SM_RECT_ONE 32

struct RectSide {
    const u8 *src;      // raw images [pairs][src_h][src_w]
    const void *map;    // [H][W][2] int32 or int16
    u8 *dst;            // rectified images [pairs][H][W]
    u8 *valid;          // [pairs][H][W] or nullptr
};

// one coordinate of a bilinear sample: the two tap positions clamped into [0, n), whether each lies inside, and the
// weight of the second
struct RectAxis {
    int c0, c1;         // clamped positions
    bool in0, in1;
    int f;              // 0 .. 31
};

__device__ __forceinline__ RectAxis rect_axis(int m, int n)
{
    RectAxis a;
    const int p = m >> SM_RECT_FRAC;                     // arithmetic shift: floor; |p| <= 2^26, p + 1 cannot overflow
    a.f = m & (SM_RECT_ONE - 1);
    a.in0 = (unsigned)p < (unsigned)n;
    a.in1 = (unsigned)(p + 1) < (unsigned)n;
    a.c0 = min(max(p, 0), n - 1);
    a.c1 = min(max(p + 1, 0), n - 1);
    return a;
}

// the nearest position floor((m + 16) / 32) without leaving 32 bits: m = 32 q + f gives q + ((f + 16) >> 5)
__device__ __forceinline__ int rect_round(int m)
{
    return (m >> SM_RECT_FRAC) + (((m & (SM_RECT_ONE - 1)) + 16) >> SM_RECT_FRAC);
}

// one destination pixel of one pair: position (mx, my) in 1/32 source pixels -> value; *ok = the validity
__device__ __forceinline__ u32 rect_sample(const u8 *__restrict__ src, int mx, int my, int src_w, int src_h, int nearest,
                                           u32 border, bool *ok)
{
    if (nearest) {
        const int xs = rect_round(mx), ys = rect_round(my);
        const bool in = (unsigned)xs < (unsigned)src_w && (unsigned)ys < (unsigned)src_h;
        const u32 v = src[(size_t)min(max(ys, 0), src_h - 1) * src_w + min(max(xs, 0), src_w - 1)];
        *ok = in;
        return in ? v : border;
    }
    const RectAxis ax = rect_axis(mx, src_w), ay = rect_axis(my, src_h);
    const u8 *r0 = src + (size_t)ay.c0 * src_w, *r1 = src + (size_t)ay.c1 * src_w;
    const u32 t00 = r0[ax.c0], t10 = r0[ax.c1], t01 = r1[ax.c0], t11 = r1[ax.c1];
    const u32 v00 = ax.in0 && ay.in0 ? t00 : border, v10 = ax.in1 && ay.in0 ? t10 : border;
    const u32 v01 = ax.in0 && ay.in1 ? t01 : border, v11 = ax.in1 && ay.in1 ? t11 : border;
    const u32 gx = SM_RECT_ONE - ax.f, gy = SM_RECT_ONE - ay.f;
    // a tap of weight 0 (f = 0) does not count: the identity map is valid up to the last row and column
    *ok = ax.in0 && ay.in0 && (ax.f == 0 || ax.in1) && (ay.f == 0 || ay.in1);
    return (gx * gy * v00 + ax.f * gy * v10 + gx * ay.f * v01 + ax.f * ay.f * v11 + 512u) >> 10;
}

// Grid: x = lanes of one image (W * H / V), y = side (0 = left, 1 = right).  REL: the map is REL16.
template <bool REL, int V>
__global__ __launch_bounds__(256) void k_rectify(RectSide left, RectSide right, int W, unsigned npx, int src_w, int src_h,
                                                 int pairs, int nearest, u32 border)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= npx / V) return;
    const RectSide s = blockIdx.y ? right : left;
    const unsigned p = t * V;
    const unsigned row = p / (unsigned)W;
    const int x = (int)(p - row * (unsigned)W), y = (int)row;
    int mx[V], my[V];
    if constexpr (REL) {
        const int16_t *m = (const int16_t *)s.map + (size_t)p * 2;
        if constexpr (V == 4) {
            const uint4 e = *(const uint4 *)m;
            const u32 w[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                mx[i] = SM_RECT_ONE * (x + i) + (int)(int16_t)(w[i] & 0xffffu);
                my[i] = SM_RECT_ONE * y + ((int)w[i] >> 16);
            }
        } else {
            mx[0] = SM_RECT_ONE * x + m[0];
            my[0] = SM_RECT_ONE * y + m[1];
        }
    } else {
        const i32 *m = (const i32 *)s.map + (size_t)p * 2;
        if constexpr (V == 4) {
            const int4 a = *(const int4 *)m, b = *(const int4 *)(m + 4);
            mx[0] = a.x; my[0] = a.y; mx[1] = a.z; my[1] = a.w;
            mx[2] = b.x; my[2] = b.y; mx[3] = b.z; my[3] = b.w;
        } else {
            mx[0] = m[0];
            my[0] = m[1];
        }
    }
    const size_t src_px = (size_t)src_w * src_h;
    for (int q = 0; q < pairs; q++) {
        const u8 *src = s.src + q * src_px;
        const size_t o = (size_t)q * npx + p;
        u32 pix = 0, val = 0;
#pragma unroll
        for (int i = 0; i < V; i++) {
            bool ok;
            pix |= rect_sample(src, mx[i], my[i], src_w, src_h, nearest, border, &ok) << (8 * i);
            val |= (u32)ok << (8 * i);
        }
        if constexpr (V == 4) {
            *(u32 *)(s.dst + o) = pix;
            if (s.valid) *(u32 *)(s.valid + o) = val;
        } else {
            s.dst[o] = (u8)pix;
            if (s.valid) s.valid[o] = (u8)val;
        }
    }
}

// sm_rectify_calib's numbers, by value
struct RectCalib {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, R[9], nfx, nfy, ncx, ncy;
};

__device__ __forceinline__ i32 rect_fixed(double u, bool bad)
{
    double t = floor(u * 32.0 + 0.5);
    t = t < -2147483648.0 ? -2147483648.0 : t;
    t = t > 2147483647.0 ? 2147483647.0 : t;
    return bad ? INT32_MIN : (i32)t;
}

// One lane per destination pixel.  tests/rectify_reference.py build_positions, line by line; nothing here may be
// contracted or reassociated.  REL: int16 displacements; one that does not fit raises *overflow (every lane that
// finds one stores the same 1: no atomic) and is stored saturated.
template <bool REL>
__global__ __launch_bounds__(256) void k_rmap_build(RectCalib c, void *map, int W, unsigned npx, i32 *overflow)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npx) return;
    const unsigned row = p / (unsigned)W;
    const int xi = (int)(p - row * (unsigned)W), yi = (int)row;
    const double xn = ((double)xi - c.ncx) / c.nfx;
    const double yn = ((double)yi - c.ncy) / c.nfy;
    const double X = (c.R[0] * xn + c.R[3] * yn) + c.R[6];
    const double Y = (c.R[1] * xn + c.R[4] * yn) + c.R[7];
    const double Z = (c.R[2] * xn + c.R[5] * yn) + c.R[8];
    const double a = X / Z;
    const double b = Y / Z;
    const double r2 = a * a + b * b;
    const double rad = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const double ad = a * rad + (((2.0 * c.p1) * a) * b + c.p2 * (r2 + (2.0 * a) * a));
    const double bd = b * rad + (c.p1 * (r2 + (2.0 * b) * b) + ((2.0 * c.p2) * a) * b);
    const double u = c.fx * ad + c.cx;
    const double v = c.fy * bd + c.cy;
    const bool bad = !(__builtin_isfinite(u) && __builtin_isfinite(v));
    const i32 mx = rect_fixed(u, bad), my = rect_fixed(v, bad);
    if constexpr (REL) {
        const long long dx = (long long)mx - SM_RECT_ONE * (long long)xi, dy = (long long)my - SM_RECT_ONE * (long long)yi;
        const long long sx = min(max(dx, -32768ll), 32767ll), sy = min(max(dy, -32768ll), 32767ll);
        if (sx != dx || sy != dy) *overflow = 1;
        int16_t *m = (int16_t *)map + (size_t)p * 2;
        m[0] = (int16_t)sx;
        m[1] = (int16_t)sy;
    } else {
        i32 *m = (i32 *)map + (size_t)p * 2;
        m[0] = mx;
        m[1] = my;
    }
}


// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static int rect_format(int map_format, const char *me, size_t *entry)
{
    if (map_format != SM_RMAP_ABS32 && map_format != SM_RMAP_REL16)
        return sm_fail(SM_ERR_ARG, "%s: map_format %d is neither SM_RMAP_ABS32 nor SM_RMAP_REL16", me, map_format);
    *entry = map_format == SM_RMAP_ABS32 ? 2 * sizeof(i32) : 2 * sizeof(int16_t);
    return SM_OK;
}

// 32 * x + dx of a REL16 map is formed in 32 bits
static int rect_plan_size(const sm_plan *plan, const char *me)
{
    if (plan->width > (1 << 25) || plan->height > (1 << 25))
        return sm_fail(SM_ERR_ARG, "%s: built for images of up to %d pixels a side (got %dx%d)", me, 1 << 25, plan->width,
                       plan->height);
    return SM_OK;
}

extern "C" int sm_rectify(sm_plan *plan, const uint8_t *d_raw_left, const uint8_t *d_raw_right, int src_w, int src_h,
                          const void *d_map_left, const void *d_map_right, int map_format, int interp, int border,
                          int pairs, uint8_t *d_left, uint8_t *d_right, uint8_t *d_valid_left, uint8_t *d_valid_right,
                          void *stream)
{
    const char *me = "sm_rectify";
    size_t entry;
    if (!d_raw_left || !d_raw_right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", me);
    if (!d_map_left || !d_map_right) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    if (!d_left || !d_right) return sm_fail(SM_ERR_ARG, "%s: output image pointer is NULL", me);
    SM_TRY(rect_format(map_format, me, &entry));
    if (interp != SM_INTERP_BILINEAR && interp != SM_INTERP_NEAREST)
        return sm_fail(SM_ERR_ARG, "%s: interp %d is neither SM_INTERP_BILINEAR nor SM_INTERP_NEAREST", me, interp);
    if (border < 0 || border > 255) return sm_fail(SM_ERR_ARG, "%s: border %d outside 0..255", me, border);
    if (src_w < 1 || src_h < 1 || (long long)src_w * src_h > INT32_MAX)
        return sm_fail(SM_ERR_ARG, "%s: source size %dx%d is not positive or has more than 2^31 - 1 pixels", me, src_w, src_h);
    // an output that IS an input or another output overlaps it whatever the sizes are (the ranges follow, with the plan)
    const void *outs[4] = {d_left, d_right, d_valid_left, d_valid_right};
    for (int i = 0; i < 4; i++) {
        if (!outs[i]) continue;
        if (outs[i] == d_raw_left || outs[i] == d_raw_right || outs[i] == d_map_left || outs[i] == d_map_right)
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input (every tap is read from the raw images)", me);
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) return sm_fail(SM_ERR_ARG, "%s: outputs overlap", me);
    }
    SM_TRY(sm_check_pairs(plan, pairs, me));
    SM_TRY(rect_plan_size(plan, me));
    if ((((uintptr_t)d_map_left | (uintptr_t)d_map_right) & (entry / 2 - 1)) != 0)
        return sm_fail(SM_ERR_ARG, "%s: a map pointer is not aligned to its %zu-byte elements", me, entry / 2);
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const size_t raw = (size_t)pairs * src_w * src_h, img = (size_t)pairs * npx, map = (size_t)npx * entry;
    for (int i = 0; i < 4; i++) {
        if (!outs[i]) continue;
        if (overlap(outs[i], d_raw_left, img, raw) || overlap(outs[i], d_raw_right, img, raw) ||
            overlap(outs[i], d_map_left, img, map) || overlap(outs[i], d_map_right, img, map))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input (every tap is read from the raw images)", me);
        for (int j = 0; j < i; j++)
            if (outs[j] && overlap(outs[i], outs[j], img)) return sm_fail(SM_ERR_ARG, "%s: outputs overlap", me);
    }
    SM_TRY(sm_use_device(plan->device));
    const RectSide l = {d_raw_left, d_map_left, d_left, d_valid_left}, r = {d_raw_right, d_map_right, d_right, d_valid_right};
    const bool vec = W % 4 == 0 && (((uintptr_t)d_map_left | (uintptr_t)d_map_right) & 15) == 0 &&
                     (((uintptr_t)d_left | (uintptr_t)d_right | (uintptr_t)d_valid_left | (uintptr_t)d_valid_right) & 3) == 0;
    const unsigned lanes = vec ? npx / 4 : npx;
    const dim3 grid((lanes + 255) / 256, 2), block(256);
#define SM_RECT_GO(REL, V) hipLaunchKernelGGL((k_rectify<REL, V>), grid, block, 0, (hipStream_t)stream, l, r, W, npx, src_w, \
                                              src_h, pairs, interp == SM_INTERP_NEAREST ? 1 : 0, (u32)border)
    if (map_format == SM_RMAP_REL16) { if (vec) SM_RECT_GO(true, 4); else SM_RECT_GO(true, 1); }
    else                             { if (vec) SM_RECT_GO(false, 4); else SM_RECT_GO(false, 1); }
#undef SM_RECT_GO
    SM_LAUNCH_CHECK("k_rectify");
    return SM_OK;
}

extern "C" int sm_rectify_map_build(sm_plan *plan, const sm_rectify_calib *calib, int map_format, void *d_map, void *stream)
{
    const char *me = "sm_rectify_map_build";
    size_t entry;
    if (!plan) return sm_fail(SM_ERR_ARG, "%s: plan is NULL", me);
    if (!calib) return sm_fail(SM_ERR_ARG, "%s: calib is NULL", me);
    if (!d_map) return sm_fail(SM_ERR_ARG, "%s: a map pointer is NULL", me);
    // every field is needed: a shorter struct is refused; of a longer (newer) one the fields this library knows are taken
    if (calib->struct_size < (int)sizeof(sm_rectify_calib))
        return sm_fail(SM_ERR_ARG, "%s: calib->struct_size %d is not that of a sm_rectify_calib (this library: %d bytes)", me,
                       calib->struct_size, (int)sizeof(sm_rectify_calib));
    SM_TRY(rect_format(map_format, me, &entry));
    SM_TRY(rect_plan_size(plan, me));
    if (((uintptr_t)d_map & (entry / 2 - 1)) != 0)
        return sm_fail(SM_ERR_ARG, "%s: the map pointer is not aligned to its %zu-byte elements", me, entry / 2);
    SM_TRY(sm_use_device(plan->device));
    hipStream_t st = (hipStream_t)stream;
    if (sm_stream_capturing(st))
        return sm_fail(SM_ERR_ARG, "%s: the stream is capturing and the builder reads a flag back (it synchronises): build "
                       "the maps before the capture begins", me);
    RectCalib c;
    c.fx = calib->fx; c.fy = calib->fy; c.cx = calib->cx; c.cy = calib->cy;
    c.k1 = calib->k1; c.k2 = calib->k2; c.p1 = calib->p1; c.p2 = calib->p2; c.k3 = calib->k3;
    for (int i = 0; i < 9; i++) c.R[i] = calib->R[i / 3][i % 3];
    c.nfx = calib->new_fx; c.nfy = calib->new_fy; c.ncx = calib->new_cx; c.ncy = calib->new_cy;
    const int W = plan->width;
    const unsigned npx = (unsigned)W * plan->height;
    const dim3 grid((npx + 255) / 256), block(256);
    if (map_format == SM_RMAP_ABS32) {
        hipLaunchKernelGGL(k_rmap_build<false>, grid, block, 0, st, c, d_map, W, npx, (i32 *)nullptr);
        SM_LAUNCH_CHECK("k_rmap_build");
        return SM_OK;
    }
    // REL16: one flag, raised by every displacement that does not fit, read back
    i32 *flag = nullptr, over = 0;
    SM_HIP(hipMalloc((void **)&flag, sizeof(i32)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(i32), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rmap_build<true>, grid, block, 0, st, c, d_map, W, npx, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&over, flag, sizeof(i32), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(flag);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "%s: building the map failed: %s", me, hipGetErrorString(e));
    if (over)
        return sm_fail(SM_ERR_ARG, "%s: a displacement of this calibration does not fit the int16 of SM_RMAP_REL16 (more than "
                       "1023 pixels, or a point at infinity): build the map with SM_RMAP_ABS32 (the contents of d_map are "
                       "not a map)", me);
    return SM_OK;
}
