// plan_dump.h -- the text form of planned geometries: what tests/golden/plan_model_parent.json.gz holds and what
// tests/helpers/plan_model_check.cpp prints.  Templates over the geometry types, so that a recording program built
// against another commit's headers prints through the same code.
#pragma once

#include <stdio.h>

#define PLAN_MATCH_FIELDS(X)                                                                                          \
    X(w) X(h) X(D) X(n) X(half) X(ext_words) X(ext_rows) X(ext_image_words) X(pad_l) X(tile_h) X(tw) X(runs) X(ds)    \
    X(nl) X(log2nl) X(threads) X(plw) X(prw) X(nsr) X(tiles_x) X(tiles_y) X(vec_ok) X(lds_bytes) X(cap2) X(duo)       \
    X(unused[0]) X(unused[1]) X(unused[2]) X(unused[3]) X(xmerge) X(xm_off) X(xm_words) X(web_bytes) X(edge_words_l)  \
    X(edge_words_r)
#define PLAN_COST_FIELDS(X)                                                                                           \
    X(w) X(h) X(D) X(ghost) X(tile_h) X(tw) X(nl) X(log2nl) X(nql) X(px) X(tiles_x) X(tiles_y) X(padl) X(lrow)       \
    X(rrow) X(nsr) X(q_tail) X(q_last) X(fast_stage) X(tbl_pad) X(lds_bytes) X(waves)

static inline unsigned plan_text_hash(const char *s)        // FNV-1a: the describe string, 32 bits of it
{
    unsigned h = 2166136261u;
    for (; *s; s++) h = (h ^ (unsigned char)*s) * 16777619u;
    return h;
}

static inline void plan_dump_names(FILE *f)
{
#define X(a) ",\"" #a "\""
    fprintf(f, "\"match_fields\":[\"kernel\",\"describe\"" PLAN_MATCH_FIELDS(X) "],\n");
    fprintf(f, "\"cost_fields\":[\"kernel\"" PLAN_COST_FIELDS(X) "],\n");
#undef X
}

// one match case: [kernel, hash of the describe string, every field of the MatchGeom]
template <class G>
static inline void plan_dump_match(FILE *f, int kernel, const char *describe, const G &g)
{
    fprintf(f, "[%d,%u", kernel, plan_text_hash(describe));
#define X(a) fprintf(f, ",%lld", (long long)g.a);
    PLAN_MATCH_FIELDS(X)
#undef X
    fprintf(f, "]");
}

// one planner's answer to a cost case: 0 (not built: the caller falls back), or [kernel, every field of the SadGeom]
template <class G>
static inline void plan_dump_cost(FILE *f, int kernel, const G &g)
{
    if (!kernel) { fprintf(f, "0"); return; }
    fprintf(f, "[%d", kernel);
#define X(a) fprintf(f, ",%d", g.a);
    PLAN_COST_FIELDS(X)
#undef X
    fprintf(f, "]");
}
