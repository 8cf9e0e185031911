// sm_near_tile_body.h -- the tile walk of the two banded data terms, included once each (no include guard) inside
//   k_census_near<NW, GHOST, MIRROR>    (sm_census_near.hip): the arg-min over a pixel's band;
//   k_sgm_near_cost<NW, GHOST, MIRROR>  (sm_sgm_near.hip): the band's costs into the banded volume.
// Both compute A_d(p), sm_census_wta's window cost, for every pixel p of a tile and every shift d of its band
// lo .. hi = the shifts of 0 .. D - 1 within `radius` of prior(p) - 1 (no band for prior(p) = 0).
//
// 256 lanes own a tile of 64 columns x 16 rows, a lane one column and four consecutive rows.  Work is spent per
// DISTINCT WANTED SHIFT OF THE TILE, not per pixel x candidate:
//   - the reference side's descriptors of the tile plus the window halo, (64 + n - 1) x (16 + n - 1) positions, are
//     dealt to the lanes, position i = tid + 256 q.  Every position is read by exactly one lane for every shift, so it
//     stays in that lane's VGPRs (at most 14 descriptors) rather than in LDS; the border rule is applied once;
//   - every lane ORs the candidate shifts of its four pixels into a D-bit mask in LDS (at most 16 dwords);
//   - the workgroup walks the set bits in ascending d (the walk is workgroup-uniform).  For each wanted d: the Hamming
//     cost of every position against the other side's descriptor at x + d (global memory: the rows sit in L2) goes to
//     LDS as u16; the horizontal n-sums of the tile's 64 columns, then the vertical n-sums (a lane slides down its four
//     rows), both u16 (A <= 48 * 625 = 30000); every pixel with d in its band takes the sum (SMN_TILE_TAKE).  The loads
//     of the next wanted shift are in flight meanwhile.
// A tile whose priors want every shift of D costs more than sm_census_wta (which shares each cost between the shifts
// of a lane and slides the window down the image), and is still exact.  LDS: (64 + n - 1)(16 + n - 1) + 64 (16 + n - 1)
// u16 and the mask, 12.2 KB at n = 25: the tile is 64 wide for every window.
//   MIRROR: the right-reference pass, as in k_census_wta: the pass's columns are read and written mirrored.
//
// The kernel has the parameters desc, prior and g (the fields of NearTileGeom, sm_census.h).  Before the include it
// defines, and after it #undefs, the places where the two differ (j = 0 .. 3: a pixel of the lane):
//   SMN_TILE_PAIR           expression: the pixels from the first pair's to this workgroup's (W, H are in scope);
//   SMN_TILE_STATE          declaration of the kernel's state per pixel, beside lo / hi;
//   SMN_TILE_NONE(j)        statement: pixel j's state before its prior is read, which a pixel without a band keeps;
//   SMN_TILE_BAND(j, s)     statement, may be empty: pixel j has a band, from the prior s;
//   SMN_TILE_SETUP          statements, may be empty: between the walk's lambdas and its first shift;
//   SMN_TILE_TAKE(j, d, a)  statement: shift d is in pixel j's band, at window cost a.  d ascends.
// Where each one stands is part of the compiled code: the kernels are instruction for instruction what they were as two
// texts with the hooks here, and not with the state declared before the include or set where it is declared (DESIGN.md
// 9a).  Behind the include ppx is SMN_TILE_PAIR, x the lane's column of the pass (it may be past W), xn its natural
// column, y0 + 4 ly + j the row of pixel j, and hi[j] >= lo[j] says that pixel j has a band.

    extern __shared__ __attribute__((aligned(16))) u32 near_lds[];
    u32 *mask = near_lds;                                                  // [16]
    unsigned short *cost = reinterpret_cast<unsigned short *>(near_lds + 16);   // [sh][sw]
    const int total = g.sw * g.sh;
    unsigned short *hs = cost + ((total + 1) & ~1);                        // [sh][64]
    const int tid = threadIdx.x, lx = tid & 63, ly = tid >> 6;
    int tx, ty;
    sm_xcd_tile(g.tiles_x, g.tiles_y, tx, ty);
    const int x0 = tx * SMN_TX, y0 = ty * SMN_TR;
    const int W = g.w, H = g.h, D = g.D, n = g.n, half = g.half;
    const size_t ppx = SMN_TILE_PAIR;                                      // pixels before this workgroup's pair
    // MIRROR: the pass's left image is mirror(R), its right image mirror(L)
    const u32 *dRef = desc + (size_t)NW * ((MIRROR ? (size_t)g.side : 0) + ppx);
    const u32 *dOth = desc + (size_t)NW * ((MIRROR ? 0 : (size_t)g.side) + ppx);

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

    // ---- this lane's four pixels: the band lo .. hi of each (hi < lo: none), the tile's mask of shifts
    if (tid < 16) mask[tid] = 0;
    __syncthreads();
    const int x = x0 + lx;                                 // column of the pass
    const int xn = MIRROR ? W - 1 - x : x;                 // natural column: prior and results
    int lo[4], hi[4];
    SMN_TILE_STATE
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + 4 * ly + j;
        lo[j] = 0;
        hi[j] = -1;
        SMN_TILE_NONE(j)
        if (x < W && y < H) {
            const int s = prior[ppx + (size_t)y * W + xn];
            // (s compared before any arithmetic on it: INT32_MIN and INT32_MAX are legal)
            if (s != 0 && s >= 1 - g.radius && s <= D + g.radius) {
                lo[j] = max(0, s - 1 - g.radius);
                hi[j] = min(D - 1, s - 1 + g.radius);
                SMN_TILE_BAND(j, s)
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
    SMN_TILE_SETUP
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
        // (lo .. hi is empty for a pixel outside the image)
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (d >= lo[j] && d <= hi[j]) { SMN_TILE_TAKE(j, d, a[j]) }
        d = d_next;
    }
