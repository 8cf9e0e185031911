// sm_census.h -- shared between the translation units of the census cost mode: sm_census.hip (transform, arg-min,
// refinement), sm_census_near.hip (the guided re-search) and sm_unique.hip (the runner-up's entry point).  Host
// declarations and constants only: the kernels stay in their units, and the other two reach the mode's argument
// checks, descriptors and launches through the functions below.
#pragma once

#include "sm_entry.h"

typedef unsigned long long u64;

#define SMN_TX 64          // transform, near: columns per workgroup
#define SMN_TR 16          // transform, near: rows per workgroup (4 per lane)

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
