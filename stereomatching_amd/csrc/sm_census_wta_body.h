// sm_census_wta_body.h -- the text of the census arg-min kernel, included twice by sm_census.hip (no include guard):
//   SMN_SECOND 0: k_census_wta<NW, GHOST, MIRROR>, token for token the kernel as it stood in sm_census.hip;
//   SMN_SECOND 1: k_census_second<NW, GHOST>, the same march for the runner-up of DESIGN.md 22: `map` is the caller's
//                 web map, and a shift within one of the map's shift at a pixel gets the bias that an out-of-range
//                 shift gets, so that it loses to every other one.  Left reference only (MIRROR = false).
// Everything the added arg-min needs sits under #if SMN_SECOND.

// what the last launch writes for a merged key A << 16 | d; SMN_SECOND: a key that still carries the bias had no shift
// to take: web2 = 0, best2 = -1
#undef SMN_KEY_WEB
#undef SMN_KEY_BEST
#if SMN_SECOND
#define SMN_KEY_WEB(k) (((k) & 0x80000000u) ? 0 : (i32)((k) & 0xffff) + 1)
#define SMN_KEY_BEST(k) (((k) & 0x80000000u) ? -1 : (i32)((k) >> 16))
#else
#define SMN_KEY_WEB(k) ((i32)((k) & 0xffff) + 1)
#define SMN_KEY_BEST(k) ((i32)((k) >> 16))
#endif

#if SMN_SECOND
template <int NW, bool GHOST>
__global__ __launch_bounds__(SMN_THREADS) void k_census_second(const u32 *__restrict__ desc,
                                                               const i32 *__restrict__ map, i32 *web, i32 *best,
                                                               const CensusGeom g)
{
    constexpr bool MIRROR = false;
#else
template <int NW, bool GHOST, bool MIRROR>
__global__ __launch_bounds__(SMN_THREADS) void k_census_wta(const u32 *__restrict__ desc, i32 *web, i32 *best,
                                                            const CensusGeom g)
{
#endif
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const int n = g.n, half = g.half;
    const int ringw = (g.lw + g.rw) * NW;                 // dwords per ring row
    u32 *ring = lds;                                      // [n + 1][lw + rw] descriptors
    u32 *X = lds + (size_t)(n + 1) * ringw;               // [4][nl][xs]: packed column sums of shifts 2k | 2k + 1
    const int tid = threadIdx.x, T = g.cg * g.nl;
    const int pair = blockIdx.z;
    int tx, ty;
    sm_xcd_tile(g.tiles_x, g.tiles_y, tx, ty);
    const int tx0 = tx * g.tw, ty0 = ty * g.th;
    const int cx0 = tx0 - 4 * g.hg;                       // image column (of the pass) of computed column 0
    const int W = g.w, H = g.h;
    const size_t npx = (size_t)W * H;
    // MIRROR: the pass's left image is mirror(R), its right image mirror(L)
    const u32 *dL = desc + (size_t)NW * ((MIRROR ? (size_t)g.side : 0) + (size_t)pair * npx);
    const u32 *dR = desc + (size_t)NW * ((MIRROR ? 0 : (size_t)g.side) + (size_t)pair * npx);

    // ---- this lane's share of a ring row: descriptor i < lw is left column cx0 + i, the others right column
    // cx0 + dlo + i - lw (columns of the pass: read mirrored under MIRROR), the border applied
    int src_col[SMN_PFMAX];
    bool src_on[SMN_PFMAX], src_r[SMN_PFMAX];
#pragma unroll
    for (int q = 0; q < SMN_PFMAX; q++) {
        const int i = tid + q * T;
        const bool is_r = i >= g.lw;
        int c = is_r ? cx0 + g.dlo + (i - g.lw) : cx0 + i;
        bool on = q < g.pf && i < g.lw + g.rw;
        if (GHOST) on = on && c >= 0 && c < W;
        else c = smn_mod(c, W);
        if (MIRROR) c = W - 1 - c;
        src_on[q] = on;
        src_r[q] = is_r;
        src_col[q] = on ? c : 0;
    }
    auto fetch = [&](int e, SmnRow<NW> &v) {
        const int y = ty0 - half + e;
        const bool vy = !GHOST || (y >= 0 && y < H);
        const int ys = GHOST ? (vy ? y : 0) : smn_mod(y, H);
#pragma unroll
        for (int q = 0; q < SMN_PFMAX; q++) {
#pragma unroll
            for (int k = 0; k < NW; k++) v.v[q][k] = 0;
            if (src_on[q] && vy) {
                const u32 *p = (src_r[q] ? dR : dL) + (size_t)NW * ((size_t)ys * W + src_col[q]);
                if constexpr (NW == 2) {
                    const uint2 t = *reinterpret_cast<const uint2 *>(p);
                    v.v[q][0] = t.x;
                    v.v[q][NW - 1] = t.y;
                } else {
                    v.v[q][0] = p[0];
                }
            }
        }
    };
    auto store = [&](int e, const SmnRow<NW> &v) {
        u32 *row = ring + (size_t)(e % (n + 1)) * ringw;
#pragma unroll
        for (int q = 0; q < SMN_PFMAX; q++) {
            const int i = tid + q * T;
            if (q < g.pf && i < g.lw + g.rw) {
                if constexpr (NW == 2) reinterpret_cast<uint2 *>(row)[i] = make_uint2(v.v[q][0], v.v[q][NW - 1]);
                else row[i] = v.v[q][0];
            }
        }
    };

    // ---- lane role: column group grp (computed columns 4 grp .. 4 grp + 3), shifts dlo + d0 .. + 7
    const int s = tid & (g.nl - 1), grp = tid >> g.log2nl;
    const int d0 = s * SMN_DS;
    const int dlim = g.dc - d0;                           // shifts of this lane inside the launch's range
    const bool out_grp = grp >= g.hg && grp < g.cg - g.hg;
    bool cin[4];                                          // ghost: computed columns outside the image sum to 0
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = cx0 + 4 * grp + j;
        cin[j] = !GHOST || (c >= 0 && c < W);
    }

    u32 P[4][SMN_DS], Q[4][SMN_DS];                       // column sums: P of the rows added, Q of the rows removed
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int dd = 0; dd < SMN_DS; dd++) { P[j][dd] = 0; Q[j][dd] = 0; }

    // Hamming costs of ring row e, added into acc: left columns 4 grp + j against right columns 4 grp + j + d0 + dd
    auto slide = [&](int e, u32 (&acc)[4][SMN_DS]) {
        const u32 *row = ring + (size_t)(e % (n + 1)) * ringw;
        const uint4 *rl = reinterpret_cast<const uint4 *>(row + (size_t)NW * 4 * grp);
        const uint4 *rr = reinterpret_cast<const uint4 *>(row + (size_t)NW * (g.lw + 4 * grp + d0));
        u32 l[4][NW], r[12][NW];
        if constexpr (NW == 2) {
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const uint4 t = rl[m];
                l[2 * m][0] = t.x; l[2 * m][NW - 1] = t.y; l[2 * m + 1][0] = t.z; l[2 * m + 1][NW - 1] = t.w;
            }
#pragma unroll
            for (int m = 0; m < 6; m++) {
                const uint4 t = rr[m];
                r[2 * m][0] = t.x; r[2 * m][NW - 1] = t.y; r[2 * m + 1][0] = t.z; r[2 * m + 1][NW - 1] = t.w;
            }
        } else {
            const uint4 t = rl[0];
            l[0][0] = t.x; l[1][0] = t.y; l[2][0] = t.z; l[3][0] = t.w;
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const uint4 u = rr[m];
                r[4 * m][0] = u.x; r[4 * m + 1][0] = u.y; r[4 * m + 2][0] = u.z; r[4 * m + 3][0] = u.w;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int dd = 0; dd < SMN_DS; dd++) {
                u32 a = acc[j][dd];
#pragma unroll
                for (int k = 0; k < NW; k++) a += (u32)__builtin_popcount(l[j][k] ^ r[j + dd][k]);   // v_bcnt_u32_b32
                acc[j][dd] = a;
            }
    };

    // ---- the march: step e brings ring row e in (rows ty0 - half + e), and row e - n leaves; from e = n - 1 on,
    // output row ty0 + e - (n - 1) is complete.  Row e + 1 is fetched at the top of step e and stored after the first
    // barrier (its ring slot held row e - n, which every lane has read by then); the second barrier publishes it and
    // the exchange rows.
    const int rows_out = min(g.th, H - ty0);
    const int steps = rows_out + n - 1;
    {
        SmnRow<NW> v0;
        fetch(0, v0);
        store(0, v0);
    }
    __syncthreads();
    for (int e = 0; e < steps; e++) {
        SmnRow<NW> nx;
        if (e + 1 < steps) fetch(e + 1, nx);
#if SMN_SECOND
        // the map's shift at the lane's four output columns of the row this step completes (requested here, used behind
        // the two barriers).  Anything outside 1 .. D (compared before any arithmetic: every int32 is legal) has no
        // neighbourhood: -4 is further than 1 from every shift.
        int dstar[4] = {-4, -4, -4, -4};
        if (out_grp && e >= n - 1) {
            const size_t mrow = ((size_t)pair * H + (size_t)(ty0 + e - (n - 1))) * W;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xj = cx0 + 4 * grp + j;
                if (xj < W) {
                    const i32 sv = map[mrow + xj];
                    dstar[j] = sv >= 1 && sv <= g.D ? sv - 1 : -4;
                }
            }
        }
#endif
        const int y_new = ty0 - half + e;
        if (!GHOST || (y_new >= 0 && y_new < H)) slide(e, P);
        if (e >= n) {
            const int y_old = y_new - n;
            if (!GHOST || (y_old >= 0 && y_old < H)) slide(e - n, Q);
        }
        const bool emit = e >= n - 1;
        __syncthreads();
        if (emit) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u32 w4[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const u32 a = P[j][2 * k] - Q[j][2 * k], b = P[j][2 * k + 1] - Q[j][2 * k + 1];
                    w4[j] = cin[j] ? (a | (b << 16)) : 0u;
                }
                *reinterpret_cast<uint4 *>(X + (size_t)(k * g.nl + s) * g.xs + 4 * grp) =
                    make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
        }
        if (e + 1 < steps) store(e + 1, nx);
        __syncthreads();
        if (!emit) continue;

        // ---- horizontal window sums (packed u16: shifts 2k | 2k + 1), first-wins keys A << 16 | d, merge over the nl
        // lanes.  A shift outside the launch's range gets 0x8000 added to its sum (A <= 30000: the field cannot wrap,
        // and the key loses to every real one).
        // (A = 30000 in a launch's first and last lane and just past its range: tests/test_census_extremes_gpu.py)
        u32 key[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        if (out_grp) {
            for (int k = 0; k < 4; k++) {
                const u32 *xr = X + (size_t)(k * g.nl + s) * g.xs + 4 * (grp - g.hg);
                // column 4 grp + j + t of the tile is xr[4 hg + j + t], t = -half .. half
                const int c0 = 4 * g.hg;
                const u16x2 inv = {(unsigned short)(2 * k < dlim ? 0 : 0x8000),
                                   (unsigned short)(2 * k + 1 < dlim ? 0 : 0x8000)};
                u16x2 S = inv;
                for (int t = -half; t <= half; t++) S += __builtin_bit_cast(u16x2, xr[c0 + t]);
                const u32 da = (u32)(g.dlo + d0 + 2 * k), db = da + 1;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (j > 0) {
                        S += __builtin_bit_cast(u16x2, xr[c0 + j + half]);
                        S -= __builtin_bit_cast(u16x2, xr[c0 + j - 1 - half]);
                    }
                    const u32 v = __builtin_bit_cast(u32, S);
#if SMN_SECOND
                    // the same bias for a shift within one of the map's, ORed in: a shift that is also outside the
                    // launch's range carries it already, and adding it twice would wrap the u16 field
                    const u32 xa = da + 1 - (u32)dstar[j] <= 2u ? 0x80000000u : 0u;
                    const u32 xb = db + 1 - (u32)dstar[j] <= 2u ? 0x80000000u : 0u;
                    key[j] = min(key[j], min((v << 16) | da | xa, (v & 0xffff0000u) | db | xb));
#else
                    key[j] = min(key[j], min((v << 16) | da, (v & 0xffff0000u) | db));
#endif
                }
            }
        }
#define SMN_MERGE(K)                                                                       \
        if (g.nl > (1 << K)) {                                                             \
            _Pragma("unroll") for (int j = 0; j < 4; j++) key[j] = min(key[j], smn_partner<K>(key[j])); \
        }
        SMN_MERGE(0) SMN_MERGE(1) SMN_MERGE(2) SMN_MERGE(3)
#undef SMN_MERGE
        if (!out_grp || s != 0) continue;
        const int y = ty0 + e - (n - 1);
        const int x = cx0 + 4 * grp;                      // first output column of the lane (pass coordinates)
        const size_t orow = ((size_t)pair * H + y) * W;
        if (g.vec_ok && x + 3 < W) {
            // natural columns x .. x + 3, or under MIRROR W - 4 - x .. W - 1 - x (reversed); both 16-byte aligned
            const size_t o = orow + (MIRROR ? (size_t)(W - 4 - x) : (size_t)x);
            u32 kk[4];
#pragma unroll
            for (int j = 0; j < 4; j++) kk[j] = key[MIRROR ? 3 - j : j];
            if (!g.first) {
                const int4 p = *reinterpret_cast<const int4 *>(web + o);
                kk[0] = min(kk[0], (u32)p.x); kk[1] = min(kk[1], (u32)p.y);
                kk[2] = min(kk[2], (u32)p.z); kk[3] = min(kk[3], (u32)p.w);
            }
            if (g.last) {
                *reinterpret_cast<int4 *>(web + o) = make_int4(SMN_KEY_WEB(kk[0]), SMN_KEY_WEB(kk[1]),
                                                               SMN_KEY_WEB(kk[2]), SMN_KEY_WEB(kk[3]));
                if (best)
                    *reinterpret_cast<int4 *>(best + o) =
                        make_int4(SMN_KEY_BEST(kk[0]), SMN_KEY_BEST(kk[1]), SMN_KEY_BEST(kk[2]), SMN_KEY_BEST(kk[3]));
            } else {
                *reinterpret_cast<int4 *>(web + o) = make_int4((i32)kk[0], (i32)kk[1], (i32)kk[2], (i32)kk[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (x + j >= W) break;
                const size_t o = orow + (MIRROR ? (size_t)(W - 1 - x - j) : (size_t)(x + j));
                u32 kj = key[j];
                if (!g.first) kj = min(kj, (u32)web[o]);
                if (g.last) {
                    web[o] = SMN_KEY_WEB(kj);
                    if (best) best[o] = SMN_KEY_BEST(kj);
                } else {
                    web[o] = (i32)kj;
                }
            }
        }
    }
}

