// sm_census_near.hip -- census cost mode, guided re-search: the arg-min of sm_census_wta over the shifts within
// `radius` of a prior map (the upsampled map of the half-resolution path), DESIGN.md 21.  It uses the census mode's
// argument checks, descriptors and descriptor layout (sm_census.h; the workspace is filled by sm_census_descriptors).
//
// PARITY UNPINNED.  Definition (A_d: sm_census_wta's window cost; prior: a web map, 1 + shift, 0 invalid; r = radius):
//   K(p) = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0;
//   K empty: web = best = 0; otherwise best = min over K of A_d(p), web = 1 + the least d of K reaching it.
//   All n x n taps of p's window take p's own d.  Right reference: mirror(near(mirror(R), mirror(L), mirror(prior))).
//
// k_census_near<NW, GHOST, MIRROR>: 256 lanes own a tile of 64 columns x 16 rows, a lane one column and four
// consecutive rows.  Work is spent per DISTINCT WANTED SHIFT OF THE TILE, not per pixel x candidate:
//   - the reference side's descriptors of the tile plus the window halo, (64 + n - 1) x (16 + n - 1) positions, are
//     dealt to the lanes, position i = tid + 256 q.  Every position is read by exactly one lane for every shift, so it
//     stays in that lane's VGPRs (at most 14 descriptors) rather than in LDS; the border rule is applied once;
//   - every lane ORs the candidate shifts of its four pixels into a D-bit mask in LDS (at most 16 dwords);
//   - the workgroup walks the set bits in ascending d (the walk is workgroup-uniform).  For each wanted d: the Hamming
//     cost of every position against the other side's descriptor at x + d (global memory: the rows sit in L2) goes to
//     LDS as u16; the horizontal n-sums of the tile's 64 columns, then the vertical n-sums (a lane slides down its four
//     rows), both u16 (A <= 48 * 625 = 30000); every pixel with d in K(p) takes min(key, A << 16 | d).  d ascends, so
//     the smaller key is "first shift wins".  The loads of the next wanted shift are in flight meanwhile.
// A tile whose priors want every shift of D costs more than sm_census_wta (which shares each cost between the shifts
// of a lane and slides the window down the image), and is still exact.  LDS: (64 + n - 1)(16 + n - 1) + 64 (16 + n - 1)
// u16 and the mask, 12.2 KB at n = 25: the tile is 64 wide for every window.
//   MIRROR: the right-reference pass, as in k_census_wta: the pass's columns are read and written mirrored.

#include "sm_device.h"
#include "sm_census.h"

#define SMN_NQ 14          // near: positions per lane at most ((64 + 24) * (16 + 24) / 256, rounded up)
#define SMN_NR 10          // near: rows of positions per wave at most ((16 + 24) / 4)

struct CensusNearGeom {
    int w, h, D;
    int n, half;
    int radius;
    int sw, sh;             // positions of a tile: 64 + n - 1 columns, 16 + n - 1 rows
    int tiles_x, tiles_y;
    long long side;         // descriptors from side 0 (left) to side 1 (right) of the workspace
};

template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(256) void k_census_near(const u32 *__restrict__ desc, const i32 *__restrict__ prior,
                                                     i32 *__restrict__ web, i32 *__restrict__ best,
                                                     const CensusNearGeom g)
{
    extern __shared__ __attribute__((aligned(16))) u32 near_lds[];
    u32 *mask = near_lds;                                                  // [16]
    unsigned short *cost = reinterpret_cast<unsigned short *>(near_lds + 16);   // [sh][sw]
    const int total = g.sw * g.sh;
    unsigned short *hs = cost + ((total + 1) & ~1);                        // [sh][64]
    const int tid = threadIdx.x, lx = tid & 63, ly = tid >> 6;
    const int pair = blockIdx.z;
    int tx, ty;
    sm_xcd_tile(g.tiles_x, g.tiles_y, tx, ty);
    const int x0 = tx * SMN_TX, y0 = ty * SMN_TR;
    const int W = g.w, H = g.h, D = g.D, n = g.n, half = g.half;
    const size_t npx = (size_t)W * H;
    // MIRROR: the pass's left image is mirror(R), its right image mirror(L)
    const u32 *dRef = desc + (size_t)NW * ((MIRROR ? (size_t)g.side : 0) + (size_t)pair * npx);
    const u32 *dOth = desc + (size_t)NW * ((MIRROR ? 0 : (size_t)g.side) + (size_t)pair * npx);

    // ---- this lane's positions: the reference descriptor, its row's offset in an image (-1: outside, ghost) and its
    // column of the pass
    u32 ref[SMN_NQ][NW];
    int prow[SMN_NQ], pcol[SMN_NQ];
#pragma unroll
    for (int q = 0; q < SMN_NQ; q++) {
        const int i = tid + 256 * q;
#pragma unroll
        for (int k = 0; k < NW; k++) ref[q][k] = 0;
        prow[q] = -1;
        pcol[q] = 0;
        if (i < total) {
            const int r = i / g.sw, c = i - r * g.sw;
            int x = x0 - half + c, y = y0 - half + r;
            bool on = true;
            if (GHOST) on = x >= 0 && x < W && y >= 0 && y < H;
            else { x = smn_mod(x, W); y = smn_mod(y, H); }
            if (on) {
                prow[q] = y * W;
                pcol[q] = x;
                const u32 *p = dRef + (size_t)NW * ((size_t)prow[q] + (MIRROR ? W - 1 - x : x));
                if constexpr (NW == 2) {
                    const uint2 t = *reinterpret_cast<const uint2 *>(p);
                    ref[q][0] = t.x;
                    ref[q][NW - 1] = t.y;
                } else {
                    ref[q][0] = p[0];
                }
            }
        }
    }

    // ---- this lane's four pixels: the candidate range lo .. hi of each (hi < lo: none), the tile's mask of shifts
    if (tid < 16) mask[tid] = 0;
    __syncthreads();
    const int x = x0 + lx;                                 // column of the pass
    const int xn = MIRROR ? W - 1 - x : x;                 // natural column: prior and results
    int lo[4], hi[4];
    u32 key[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + 4 * ly + j;
        lo[j] = 0;
        hi[j] = -1;
        key[j] = 0xffffffffu;
        if (x < W && y < H) {
            const int s = prior[(size_t)pair * npx + (size_t)y * W + xn];
            // (s compared before any arithmetic on it: INT32_MIN and INT32_MAX are legal)
            if (s != 0 && s >= 1 - g.radius && s <= D + g.radius) {
                lo[j] = max(0, s - 1 - g.radius);
                hi[j] = min(D - 1, s - 1 + g.radius);
                const u64 bits = ((1ull << (hi[j] - lo[j] + 1)) - 1) << (lo[j] & 31);   // at most 9 bits
                atomicOr(&mask[lo[j] >> 5], (u32)bits);
                if ((u32)(bits >> 32)) atomicOr(&mask[(lo[j] >> 5) + 1], (u32)(bits >> 32));
            }
        }
    }
    __syncthreads();

    // ---- the wanted shifts in ascending order.  The other side's descriptors of the NEXT wanted shift are requested
    // before the barriers of the current one, all of a lane's positions back to back: their latency (a trip to L2 per
    // position, were they loaded where they are used) passes behind the two sums.
    const int words = (D + 31) >> 5;
    int wd = -1;
    u32 m = 0;
    auto next_wanted = [&]() -> int {                      // workgroup-uniform
        while (m == 0) {
            if (++wd >= words) return -1;
            m = __builtin_amdgcn_readfirstlane(mask[wd]);
        }
        const int d = 32 * wd + __builtin_ctz(m);
        m &= m - 1;
        return d;
    };
    u32 oth[SMN_NQ][NW];
    // every lane loads for every q below the tile's count: a position that has no descriptor to load (outside the
    // image, past the ghost border, or past the last position) reads descriptor 0 of the pair and ignores it
    auto request = [&](int d) {
        const int dm = GHOST ? d : d % W;                  // toroidal: x + d mod W by one conditional subtraction
#pragma unroll
        for (int q = 0; q < SMN_NQ; q++) {
            if (256 * q >= total) break;
            int xo = pcol[q] + dm;
            bool on = prow[q] >= 0;
            if (GHOST) on = on && xo < W;
            else if (xo >= W) xo -= W;
            const size_t off = on ? (size_t)prow[q] + (size_t)(MIRROR ? W - 1 - xo : xo) : 0;
            const u32 *p = dOth + (size_t)NW * off;
            if constexpr (NW == 2) {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                oth[q][0] = v.x;
                oth[q][NW - 1] = v.y;
            } else {
                oth[q][0] = p[0];
            }
        }
    };
    int d = next_wanted();
    if (d >= 0) request(d);
    while (d >= 0) {
        // Hamming costs of the positions
#pragma unroll
        for (int q = 0; q < SMN_NQ; q++) {
            if (256 * q >= total) break;
            const int i = tid + 256 * q;
            const bool past = GHOST && pcol[q] + d >= W;   // ghost: C = 0 past the right border
            u32 c = 0;
#pragma unroll
            for (int k = 0; k < NW; k++) c += (u32)__builtin_popcount(ref[q][k] ^ (past ? 0u : oth[q][k]));
            if (i < total) cost[i] = (unsigned short)(prow[q] >= 0 ? c : 0u);
        }
        const int d_next = next_wanted();
        if (d_next >= 0) request(d_next);
        __syncthreads();
        // horizontal n-sums of the tile's columns, every row of the positions: rows ly, ly + 4, ... of a lane (ly is the
        // wave's number, so the row tests are scalar), summed side by side so that their LDS reads are in flight
        // together and not one behind the other's wait
        {
            u32 s[SMN_NR];
#pragma unroll
            for (int k = 0; k < SMN_NR; k++) s[k] = 0;
            const unsigned short *cr = cost + ly * g.sw + lx;
#pragma unroll 3
            for (int t = 0; t < n; t++) {
#pragma unroll
                for (int k = 0; k < SMN_NR; k++)
                    if (ly + 4 * k < g.sh) s[k] += cr[4 * k * g.sw + t];
            }
#pragma unroll
            for (int k = 0; k < SMN_NR; k++)
                if (ly + 4 * k < g.sh) hs[(ly + 4 * k) * 64 + lx] = (unsigned short)s[k];
        }
        __syncthreads();
        // vertical n-sums: rows 4 ly .. 4 ly + 3 of the tile.  Row j's sum is rows j .. j + n - 1 of hs: the four share
        // rows 3 .. n - 1 (n >= 4), summed once; for n < 4 each is summed on its own
        const unsigned short *hc = hs + (4 * ly) * 64 + lx;
        u32 a[4];
        if (n >= 4) {
            u32 mid = 0;
#pragma unroll 4
            for (int t = 3; t < n; t++) mid += hc[t * 64];
            const u32 h0 = hc[0], h1 = hc[64], h2 = hc[128];
            const u32 t0 = hc[n * 64], t1 = hc[(n + 1) * 64], t2 = hc[(n + 2) * 64];
            a[0] = h0 + h1 + h2 + mid;
            a[1] = h1 + h2 + mid + t0;
            a[2] = h2 + mid + t0 + t1;
            a[3] = mid + t0 + t1 + t2;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                a[j] = 0;
                for (int t = 0; t < n; t++) a[j] += hc[(j + t) * 64];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (d >= lo[j] && d <= hi[j]) key[j] = min(key[j], (a[j] << 16) | (u32)d);
        d = d_next;
    }

    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + 4 * ly + j;
        if (y >= H) break;
        const size_t o = (size_t)pair * npx + (size_t)y * W + xn;
        const bool any = hi[j] >= lo[j];
        web[o] = any ? (i32)(key[j] & 0xffff) + 1 : 0;
        if (best) best[o] = any ? (i32)(key[j] >> 16) : 0;
    }
}

// the re-search from the workspace's descriptors
static int near_launch(const sm_plan *plan, int cw, bool mirror, int pairs, const i32 *d_prior, int radius, i32 *d_web,
                       i32 *d_best, hipStream_t st)
{
    CensusNearGeom g;
    g.w = plan->width; g.h = plan->height; g.D = plan->num_shifts;
    g.half = plan->square_width / 2; g.n = 2 * g.half + 1;
    g.radius = radius;
    g.sw = SMN_TX + g.n - 1;
    g.sh = SMN_TR + g.n - 1;
    g.tiles_x = (g.w + SMN_TX - 1) / SMN_TX;
    g.tiles_y = (g.h + SMN_TR - 1) / SMN_TR;
    g.side = (long long)plan->max_pairs * g.w * g.h;
    const int total = g.sw * g.sh;
    const size_t lds = 4 * 16 + 2 * ((size_t)((total + 1) & ~1) + (size_t)g.sh * 64);
    if (total > 256 * SMN_NQ || lds > 64 * 1024)
        return sm_fail(SM_ERR_HIP, "census near: internal tiling error (%d positions, %zu bytes of LDS)", total, lds);
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = cw == 7 ? SM_PASS_KERNEL(k_census_near, 2, ghost, mirror) : SM_PASS_KERNEL(k_census_near, 1, ghost, mirror);
    void *args[] = {(void *)&plan->d_census, (void *)&d_prior, (void *)&d_web, (void *)&d_best, (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y, pairs), dim3(256), args, lds, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_census_near failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// what the three entries check besides their pointers: the radius (which needs no plan) and sm_census_args; then every
// output against the images and the priors
static int near_args(const sm_plan *plan, int census_width, int pairs, int radius, const char *me)
{
    if (radius < 1 || radius > 4) return sm_fail(SM_ERR_ARG, "%s: radius %d outside 1..4", me, radius);
    return sm_census_args(plan, census_width, pairs, me);
}

static int near_inputs_apart(const sm_plan *plan, int pairs, const uint8_t *left, const uint8_t *right,
                             const i32 *prior_a, const i32 *prior_b, const i32 *const *outs, int n_outs,
                             const i32 *rejected, const char *me)
{
    const size_t px = (size_t)pairs * plan->width * plan->height, map = px * sizeof(i32);
    for (int k = 0; k <= n_outs; k++) {
        const void *o = k < n_outs ? (const void *)outs[k] : (const void *)rejected;
        const size_t ob = k < n_outs ? map : (size_t)pairs * sizeof(i32);
        if (!o) continue;
        if (overlap(o, left, ob, px) || overlap(o, right, ob, px))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input image", me);
        if ((prior_a && overlap(o, prior_a, ob, map)) || (prior_b && overlap(o, prior_b, ob, map)))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps a prior map", me);
    }
    return SM_OK;
}

// the mode as the entry driver sees it (sm_entry.h): the census mode with a prior map for each direction the call runs
struct CensusNearMode : CensusMode {
    int radius;
    const i32 *prior, *prior_right;
    CensusNearMode(int census_width, int radius_, const i32 *p, const i32 *p_right)
        : CensusMode(census_width), radius(radius_), prior(p), prior_right(p_right) {}
    int inputs(const sm_call &c, bool left, bool right) const
    {
        if (left && right)
            return prior && prior_right ? SM_OK : sm_fail(SM_ERR_ARG, "%s: prior map pointer is NULL", c.me);
        return (right ? prior_right : prior) ? SM_OK
               : sm_fail(SM_ERR_ARG, "%s: %s is NULL", c.me, right ? "d_prior_right" : "d_prior");
    }
    int args(const sm_call &c) const { return near_args(c.plan, cw, c.pairs, radius, c.me); }
    int apart(const sm_call &c, const i32 *const *outs, int n_outs, const i32 *rejected) const
    {
        return near_inputs_apart(c.plan, c.pairs, c.left, c.right, prior, prior_right, outs, n_outs, rejected, c.me);
    }
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *) const
    {
        return near_launch(c.plan, cw, mirror, c.pairs, mirror ? prior_right : prior, radius, web, best, c.st);
    }
};

extern "C" int sm_census_wta_near(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                  int census_width, int pairs, const int32_t *d_prior, int radius, int32_t *d_web,
                                  int32_t *d_best, void *stream)
{
    return sm_entry_one({"sm_census_wta_near", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CensusNearMode(census_width, radius, d_prior, nullptr), false, d_web, d_best, nullptr);
}

extern "C" int sm_census_wta_near_right(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                        int census_width, int pairs, const int32_t *d_prior_right, int radius,
                                        int32_t *d_web_right, int32_t *d_best_right, void *stream)
{
    return sm_entry_one({"sm_census_wta_near_right", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                        CensusNearMode(census_width, radius, nullptr, d_prior_right), true, d_web_right, d_best_right,
                        nullptr);
}

extern "C" int sm_census_near_lr(sm_plan *plan, const uint8_t *d_gray_left, const uint8_t *d_gray_right,
                                 int census_width, int pairs, const int32_t *d_prior, const int32_t *d_prior_right,
                                 int radius, int max_diff, int32_t *d_web, int32_t *d_best, int32_t *d_web_right,
                                 int32_t *d_rejected, void *stream)
{
    return sm_entry_lr({"sm_census_near_lr", plan, d_gray_left, d_gray_right, pairs, (hipStream_t)stream},
                       CensusNearMode(census_width, radius, d_prior, d_prior_right), max_diff, d_web, d_best,
                       d_web_right, d_rejected, nullptr);
}
