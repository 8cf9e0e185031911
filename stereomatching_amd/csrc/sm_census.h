// sm_census.h -- shared between the translation units of the census cost mode: sm_census.hip (transform, arg-min,
// refinement), sm_census_near.hip (the guided re-search) and sm_unique.hip (the runner-up's entry point), and with
// sm_sgm_near.hip, whose data term is the guided re-search's.  Host declarations and constants only: the kernels stay
// in their units (a text two units share: sm_near_tile_body.h), and the others reach the mode's argument checks,
// descriptors and launches through the functions below.
#pragma once

#include "sm_entry.h"

typedef unsigned long long u64;

#define SMN_TX 64          // transform, near: columns per workgroup
#define SMN_TR 16          // transform, near: rows per workgroup (4 per lane)
#define SMN_NQ 14          // near: positions per lane at most ((64 + 24) * (16 + 24) / 256, rounded up)
#define SMN_NR 10          // near: rows of positions per wave at most ((16 + 24) / 4)

// sm_census.hip.  (sm_census_descriptors, which SGM calls as well, is declared in sm_internal.h.)
// what every census entry checks besides its pointers (before any device call)
int sm_census_args(const sm_plan *plan, int census_width, int pairs, const char *me);
// the arg-min over the plan's shifts from the workspace's descriptors
int sm_census_wta_launch(const sm_plan *plan, int cw, bool mirror, int pairs, i32 *d_web, i32 *d_best, hipStream_t st);
// the runner-up against the web map d_map (k_census_second, for sm_unique.hip): the same arg-min without the shifts
// within one of the map's; web2 = 0 and best2 = -1 where none is left
int sm_census_second_launch(const sm_plan *plan, int cw, int pairs, const i32 *d_map, i32 *d_web2, i32 *d_best2,
                            hipStream_t st);

// the mode as the entry driver sees it (sm_entry.h)
struct CensusMode : sm_mode {
    static constexpr const sm_ws_set &ws = SM_WS_SET_CENSUS;
    int cw;
    explicit CensusMode(int census_width) : cw(census_width) {}
    int args(const sm_call &c) const { return sm_census_args(c.plan, cw, c.pairs, c.me); }
    int prepare(const sm_call &c) const { return sm_census_descriptors(c.plan, cw, c.left, c.right, c.pairs, c.st); }
    int pass(const sm_call &c, bool mirror, i32 *web, i32 *best, int16_t *) const
    {
        return sm_census_wta_launch(c.plan, cw, mirror, c.pairs, web, best, c.st);
    }
};

// sm_census_near.hip, for banded SGM (sm_sgm_near.hip) as well: what the two data terms over the shifts within `radius`
// of a prior map share besides their kernel text (sm_near_tile_body.h).
// The tile walk's view of a plan: the first fields of both kernels' parameter structs
struct NearTileGeom {
    int w, h, D;
    int n, half;
    int radius;
    int sw, sh;             // positions of a tile: 64 + n - 1 columns, 16 + n - 1 rows
    int tiles_x, tiles_y;
    long long side;         // descriptors from side 0 (left) to side 1 (right) of the census workspace
};
// fills *g and the LDS bytes of a launch; refuses, as `what` ("census near", "sgm near"), a tile the kernels cannot hold
int sm_near_tile_geom(const sm_plan *plan, int radius, const char *what, NearTileGeom *g, size_t *lds);
// the prior maps of a call (one for each direction it runs) and its radius: a base of both modes
struct NearPriors {
    int radius;
    const i32 *prior, *prior_right;
    int inputs(const sm_call &c, bool left, bool right) const;
    int radius_arg(const char *me) const;               // outside 1..4 (needs no plan)
    // every output against the images and the priors: the int32 maps, the counts, and one more output of another size
    int apart(const sm_call &c, const i32 *const *outs, int n_outs, const i32 *rejected, const void *extra = nullptr,
              size_t extra_bytes = 0) const;
};
