// sm_entry.h -- one driver for the left, right and checked entry points of every cost mode.
// Included by the units that define a mode (sm_census.hip and sm_census_near.hip through sm_census.h, sm_sgm.hip, sm_lr.hip); an entry
// point is one call of sm_entry_one or sm_entry_lr with the call's arguments and the mode's description.
#pragma once

#include "sm_internal.h"

// the arguments every entry takes
struct sm_call {
    const char *me;                     // the entry point's name, for messages
    sm_plan *plan;
    const uint8_t *left, *right;        // the gray images
    int pairs;
    hipStream_t st;
};

// A mode's description is a struct that holds the call's mode arguments and derives from this one.  It has
//   ws                              the workspace set
//   args(c)                         the scalar checks, those that need no plan first (it is where a NULL plan is refused)
//   prepare(c)                      what both directions share, launched once
//   pass(c, mirror, web, best, sub) one direction: mirror = the right-reference pass
// and replaces the members below where it differs.
struct sm_mode {
    // the order in which the right-reference pass leaves its map.  Natural: the checked entry has it written into the
    // caller's d_web_right (or the plan's d_web_lr as scratch) and the check gathers from it.  Mirrored: the pass always
    // writes into d_web_lr, the check writes d_web_right, and the single right entry turns its maps round in place.
    static constexpr bool right_mirrored = false;
    // the single entries' overlap refusal names its two maps (the modes differ here: SGM says "result maps overlap")
    static constexpr bool overlap_names_maps = true;
    // the mode's own input pointers, checked between the images and d_web
    int inputs(const sm_call &, bool, bool) const { return SM_OK; }
    // outputs against inputs, after the map overlaps (the modes differ here: only the guided re-search checks its
    // outputs against the input images)
    int apart(const sm_call &, const i32 *const *, int, const i32 *) const { return SM_OK; }
    int prepare(const sm_call &) const { return SM_OK; }
};

// The order of the checks is behaviour (the first failure is the message): pointers, max_diff, the mode's scalars, map
// overlaps, outputs against inputs; only then the device and the workspace.  A refused call has made no device call.

// one direction: the left maps, or (right) the right-reference maps.  d_best and d_sub may be NULL.
template <class Mode>
static int sm_entry_one(const sm_call &c, const Mode &m, bool right, i32 *d_web, i32 *d_best, int16_t *d_sub)
{
    const char *web = right ? "d_web_right" : "d_web", *best = right ? "d_best_right" : "d_best";
    if (!c.left || !c.right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", c.me);
    SM_TRY(m.inputs(c, !right, right));
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: %s is NULL", c.me, web);
    SM_TRY(m.args(c));
    const size_t map = (size_t)c.pairs * c.plan->width * c.plan->height * sizeof(i32);
    if ((d_best && overlap(d_web, d_best, map)) || (d_sub && overlap(d_sub, d_web, map / 2, map)) ||
        (d_sub && d_best && overlap(d_sub, d_best, map / 2, map)))
        return m.overlap_names_maps ? sm_fail(SM_ERR_ARG, "%s: %s and %s overlap", c.me, web, best)
                                    : sm_fail(SM_ERR_ARG, "%s: result maps overlap", c.me);
    const i32 *outs[] = {d_web, d_best};
    SM_TRY(m.apart(c, outs, 2, nullptr));
    SM_TRY(sm_use_device(c.plan->device));
    SM_TRY(sm_ws_need(c.plan, m.ws, c.st, c.me));
    SM_TRY(m.prepare(c));
    SM_TRY(m.pass(c, right, d_web, d_best, d_sub));
    return right && m.right_mirrored ? sm_lr_unmirror(c.plan, c.pairs, d_web, d_best, c.st) : SM_OK;
}

// both directions and the check: d_web is the checked map.  d_best, d_web_right, d_rejected and d_sub may be NULL.
template <class Mode>
static int sm_entry_lr(const sm_call &c, const Mode &m, int max_diff, i32 *d_web, i32 *d_best, i32 *d_web_right,
                       i32 *d_rejected, int16_t *d_sub)
{
    if (!c.left || !c.right) return sm_fail(SM_ERR_ARG, "%s: input image pointer is NULL", c.me);
    SM_TRY(m.inputs(c, true, true));
    if (!d_web) return sm_fail(SM_ERR_ARG, "%s: d_web is NULL", c.me);
    if (max_diff < 0) return sm_fail(SM_ERR_ARG, "%s: max_diff %d is negative", c.me, max_diff);
    SM_TRY(m.args(c));
    SM_TRY(sm_check_lr_maps(c.plan, c.pairs, d_web, d_best, d_web_right, d_sub, d_rejected, c.me));
    const i32 *outs[] = {d_web, d_best, d_web_right};
    SM_TRY(m.apart(c, outs, 3, d_rejected));
    SM_TRY(sm_use_device(c.plan->device));
    SM_TRY(sm_ws_need(c.plan, m.ws, c.st, c.me));
    // what both directions share once (the census descriptors), the left pass, the right-reference pass into `right`
    // (natural order: the caller's map, or the plan's mirrored-order map used as scratch), then the check, which
    // gathers from it; a subpixel map of the left pass is zeroed where the check rejected
    i32 *right = m.right_mirrored || !d_web_right ? c.plan->d_web_lr : d_web_right;
    SM_TRY(m.prepare(c));
    SM_TRY(m.pass(c, false, d_web, d_best, d_sub));
    SM_TRY(m.pass(c, true, right, nullptr, nullptr));
    SM_TRY(sm_lr_check_launch(c.plan, m.right_mirrored, d_web, right, d_web, m.right_mirrored ? d_web_right : nullptr,
                              d_rejected, max_diff, c.pairs, c.st));
    return d_sub ? sm_sub_mask_launch(d_web, d_sub, (long long)c.pairs * c.plan->width * c.plan->height, c.st) : SM_OK;
}
