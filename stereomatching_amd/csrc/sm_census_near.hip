// sm_census_near.hip -- census cost mode, guided re-search: the arg-min of sm_census_wta over the shifts within
// `radius` of a prior map (the upsampled map of the half-resolution path), DESIGN.md 21.  It uses the census mode's
// argument checks, descriptors and descriptor layout (sm_census.h; the workspace is filled by sm_census_descriptors).
//
// PARITY UNPINNED.  Definition (A_d: sm_census_wta's window cost; prior: a web map, 1 + shift, 0 invalid; r = radius):
//   K(p) = { d : 0 <= d <= D - 1, |d - (prior(p) - 1)| <= r }, empty for prior(p) = 0;
//   K empty: web = best = 0; otherwise best = min over K of A_d(p), web = 1 + the least d of K reaching it.
//   All n x n taps of p's window take p's own d.  Right reference: mirror(near(mirror(R), mirror(L), mirror(prior))).
//
// k_census_near<NW, GHOST, MIRROR>: the tile walk of sm_near_tile_body.h (a 64 x 16 tile's positions in registers, the
// OR of the wanted shifts in LDS, a uniform walk of its set bits, row sums then column sums through LDS), which banded
// SGM's data term shares.  Here every pixel with d in K(p) takes min(key, A << 16 | d): d ascends, so the smaller key is
// "first shift wins".

#include "sm_device.h"
#include "sm_census.h"

struct CensusNearGeom : NearTileGeom {};

template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(256) void k_census_near(const u32 *__restrict__ desc, const i32 *__restrict__ prior,
                                                     i32 *__restrict__ web, i32 *__restrict__ best,
                                                     const CensusNearGeom g)
{
    const int pair = blockIdx.z;
#define SMN_TILE_PAIR ((size_t)pair * ((size_t)W * H))
#define SMN_TILE_STATE u32 key[4];                         // the least A << 16 | d so far
#define SMN_TILE_NONE(j) key[j] = 0xffffffffu;
#define SMN_TILE_BAND(j, s)
#define SMN_TILE_SETUP
#define SMN_TILE_TAKE(j, d, a) key[j] = min(key[j], ((a) << 16) | (u32)(d));
#include "sm_near_tile_body.h"
#undef SMN_TILE_PAIR
#undef SMN_TILE_STATE
#undef SMN_TILE_NONE
#undef SMN_TILE_BAND
#undef SMN_TILE_SETUP
#undef SMN_TILE_TAKE

    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + 4 * ly + j;
        if (y >= H) break;
        const size_t o = ppx + (size_t)y * W + xn;
        const bool any = hi[j] >= lo[j];
        web[o] = any ? (i32)(key[j] & 0xffff) + 1 : 0;
        if (best) best[o] = any ? (i32)(key[j] >> 16) : 0;
    }
}

// the tile geometry both data terms launch with
int sm_near_tile_geom(const sm_plan *plan, int radius, const char *what, NearTileGeom *g, size_t *lds)
{
    g->w = plan->width; g->h = plan->height; g->D = plan->num_shifts;
    g->half = plan->square_width / 2; g->n = 2 * g->half + 1;
    g->radius = radius;
    g->sw = SMN_TX + g->n - 1;
    g->sh = SMN_TR + g->n - 1;
    g->tiles_x = (g->w + SMN_TX - 1) / SMN_TX;
    g->tiles_y = (g->h + SMN_TR - 1) / SMN_TR;
    g->side = (long long)plan->max_pairs * g->w * g->h;
    const int total = g->sw * g->sh;
    *lds = 4 * 16 + 2 * ((size_t)((total + 1) & ~1) + (size_t)g->sh * 64);
    if (total > 256 * SMN_NQ || *lds > 64 * 1024)
        return sm_fail(SM_ERR_HIP, "%s: internal tiling error (%d positions, %zu bytes of LDS)", what, total, *lds);
    return SM_OK;
}

// the re-search from the workspace's descriptors
static int near_launch(const sm_plan *plan, int cw, bool mirror, int pairs, const i32 *d_prior, int radius, i32 *d_web,
                       i32 *d_best, hipStream_t st)
{
    CensusNearGeom g;
    size_t lds;
    SM_TRY(sm_near_tile_geom(plan, radius, "census near", &g, &lds));
    const bool ghost = plan->border == SM_GHOST;
    const void *fn = cw == 7 ? SM_PASS_KERNEL(k_census_near, 2, ghost, mirror) : SM_PASS_KERNEL(k_census_near, 1, ghost, mirror);
    void *args[] = {(void *)&plan->d_census, (void *)&d_prior, (void *)&d_web, (void *)&d_best, (void *)&g};
    const hipError_t e = hipLaunchKernel(fn, dim3(g.tiles_x, g.tiles_y, pairs), dim3(256), args, lds, st);
    if (e != hipSuccess) return sm_fail(SM_ERR_HIP, "launch of k_census_near failed: %s", hipGetErrorString(e));
    return SM_OK;
}

// the checks of the prior maps and the radius, for banded SGM's mode as well: one copy of each message (where they
// stand in the order of an entry's checks is the driver's and the modes' business, sm_entry.h)
int NearPriors::inputs(const sm_call &c, bool left, bool right) const
{
    if (left && right)
        return prior && prior_right ? SM_OK : sm_fail(SM_ERR_ARG, "%s: prior map pointer is NULL", c.me);
    return (right ? prior_right : prior) ? SM_OK
           : sm_fail(SM_ERR_ARG, "%s: %s is NULL", c.me, right ? "d_prior_right" : "d_prior");
}

int NearPriors::radius_arg(const char *me) const
{
    return radius < 1 || radius > 4 ? sm_fail(SM_ERR_ARG, "%s: radius %d outside 1..4", me, radius) : SM_OK;
}

int NearPriors::apart(const sm_call &c, const i32 *const *outs, int n_outs, const i32 *rejected, const void *extra,
                      size_t extra_bytes) const
{
    const size_t px = (size_t)c.pairs * c.plan->width * c.plan->height, map = px * sizeof(i32);
    for (int k = 0; k <= n_outs + 1; k++) {
        const void *o = k < n_outs ? (const void *)outs[k] : k == n_outs ? (const void *)rejected : extra;
        const size_t ob = k < n_outs ? map : k == n_outs ? (size_t)c.pairs * sizeof(i32) : extra_bytes;
        if (!o) continue;
        if (overlap(o, c.left, ob, px) || overlap(o, c.right, ob, px))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps an input image", c.me);
        if ((prior && overlap(o, prior, ob, map)) || (prior_right && overlap(o, prior_right, ob, map)))
            return sm_fail(SM_ERR_ARG, "%s: an output overlaps a prior map", c.me);
    }
    return SM_OK;
}

// the mode as the entry driver sees it (sm_entry.h): the census mode with a prior map for each direction the call runs.
// Besides their pointers the three entries check the radius (which needs no plan) and sm_census_args; then every output
// against the images and the priors
struct CensusNearMode : CensusMode, NearPriors {
    using NearPriors::inputs;
    using NearPriors::apart;
    CensusNearMode(int census_width, int radius_, const i32 *p, const i32 *p_right)
        : CensusMode(census_width), NearPriors{radius_, p, p_right} {}
    int args(const sm_call &c) const
    {
        SM_TRY(radius_arg(c.me));
        return sm_census_args(c.plan, cw, c.pairs, c.me);
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
