// sm_bs_network.h -- the window-sum update of the bit-sliced match kernel as ONE signed
// carry-save network:
//
//     S' = S + sum_i e_i - sum_i l_i          e_i: the N mismatch bits of the entering row,
//                                             l_i: those of the leaving row, S on SB planes
//
// The N entering bits go in as wires of weight 1 and sign +, the N leaving bits as wires of
// weight 1 and sign -, plane k of S as a + wire of weight 2^k.  Every weight is reduced to a
// single wire with 3:2 cells; a cell is two v_bitop3, sum a ^ b ^ c and a carry whose
// immediate complements the negative inputs:
//     a + b + c =   (a^b^c) + 2 maj(a, b, c)
//     a + b - c = - (a^b^c) + 2 maj(a, b, ~c)
//     a - b - c =   (a^b^c) - 2 maj(~a, b, c)
//   - a - b - c = - (a^b^c) - 2 maj(a, b, c)
// Two wires left over take a half adder (a - b = (a^b) - 2 (~a & b)).  A last wire -s of a
// weight w is the same as +s at w and -s at 2w: the plane is s, and the wire goes on to the
// next weight with no instruction.  Wires above plane SB - 1 are dropped and the top plane is
// the xor of its wires: 0 <= S' <= N * N < 2^SB is known, and the sum is right modulo 2^SB.
//
// The wiring is made at compile time (net_plan), the same for the device, where it is unrolled
// into IT items side by side like the other lockstep forms of sm_match_bs_kernel.h, and for the
// host (-DSM_BS_NETWORK_HOST: bop<IMM> in plain C++), where tests/helpers/bs_network_check.cpp
// runs it against integer arithmetic.  net_plan also counts the operations, next to those of the
// forms it replaces (two count_lockstep trees + addsub_lockstep): net_ops / net_ops_separate.
//
// GROUPED inputs (GR).  The sum bit of a first cell over three columns c, c + 1, c + 2 of ONE row,
//     s = x_c ^ x_c+1 ^ x_c+2 = (L_c ^ L_c+1 ^ L_c+2) ^ (R_c+d ^ R_c+1+d ^ R_c+2+d) = LX_c ^ RX_c+d,
// needs none of the three mismatch bits: LX is shared by every shift of the row and RX_u by every (c, d) with
// c + d = u.  Its carry needs two of them, maj(x_c, x_c+1, x_c+2) = maj(x_c, x_c+1, ~s).  So of every three
// columns of a row side the third input is the PARITY of the group, handed in like a bit, and a carry-only cell
// turns (x_c, x_c+1, parity) into the wire of weight 2; the parity itself is the wire of weight 1.  Both carry the
// sign of their row.  floor(N / 3) groups per row side, the N mod 3 columns left over stay single bits: one
// operation fewer per group, net_ops<N, true>() == net_ops<N>() - 2 * (N / 3).
#pragma once

#ifdef SM_BS_NETWORK_HOST
#include <cstdint>
typedef uint32_t u32;
#define SM_NET_FN inline
#define SM_NET_UNROLL
#define SM_PIN() do { } while (0)
#define SM_SYNC() do { } while (0)
template <int IMM>
inline u32 bop(u32 a, u32 b, u32 c)      // bit (a<<2|b<<1|c) of IMM, like v_bitop3_b32
{
    u32 r = 0;
    for (int k = 0; k < 8; k++)
        if ((IMM >> k) & 1) r |= ((k & 4) ? a : ~a) & ((k & 2) ? b : ~b) & ((k & 1) ? c : ~c);
    return r;
}
#else
#define SM_NET_FN __device__ __forceinline__
#define SM_NET_UNROLL _Pragma("unroll")
#endif

#include "sm_bs_ops.h"      // BOP_XOR3, BOP_MAJ, BOP_MAJ_NC, BOP_BORROW (= maj(~a, b, c)), BOP_ANDN; bits_for

// one cell: inputs a, b, c (wire numbers; c < 0: a half adder, b < 0 as well: none), the wire
// of its sum and of its carry (< 0: not made), and the immediate of the carry
// grp: the carry-only cell of a group of three columns: a, b are two of its bits, c is its parity, which IS the
// sum -- wire s is c under another number, no operation
struct NetCell { short a, b, c, s, cy; short imm; short w; bool grp = false; };

// Wire numbers: [0, N) entering bits, [N, 2N) leaving bits, [2N, 2N + SB) the planes of S,
// from 2N + SB on the outputs of the cells in the order they are made.  Grouped: inputs 3g, 3g + 1 of a row
// side are the first two bits of group g and input 3g + 2 is its parity, g < N / 3.
template <int N, int SB>
struct NetPlan {
    static constexpr int NIN = 2 * N + SB;
    static constexpr int MAXC = 2 * N + 2 * SB;     // every full adder removes a wire; half adders: one per weight
    NetCell cell[MAXC] = {};
    int ncell = 0;
    int nwires = NIN;
    int nops = 0;
    short out[SB] = {};         // the wire that is plane k of S'
};

template <int N, int SB, bool GR = false>
constexpr NetPlan<N, SB> net_make_plan()
{
    NetPlan<N, SB> p;
    constexpr int G = GR ? N / 3 : 0;
    // The wires of a weight are reduced as a CHAIN: a cell takes the sum of the cell before it and
    // two fresh wires, so one partial sum per weight is alive, not a level of a tree.
    short q[4 * N + 4 * SB] = {}, nx[2 * N + 2 * SB] = {};
    bool qneg[4 * N + 4 * SB] = {}, nxneg[2 * N + 2 * SB] = {};
    short qgrp[4 * N + 4 * SB] = {};    // 1 + first input of a group whose carry-only cell is still to be made
    int head = 0, tail = 0, nn = 0;
    for (int w = 0; w < SB; w++) {
        const bool top = w == SB - 1;
        head = 0; tail = 0;
        q[tail] = (short)(2 * N + w); qneg[tail++] = false;          // plane w of S: ready from the start
        if (w == 0) {
            for (int g = 0; g < G; g++) {                            // entering and leaving groups by turns
                qgrp[tail] = (short)(1 + 3 * g); qneg[tail++] = false;
                qgrp[tail] = (short)(1 + N + 3 * g); qneg[tail++] = true;
            }
            for (int i = 3 * G; i < N; i++) {                        // entering and leaving bits by turns
                q[tail] = (short)i; qneg[tail++] = false;
                q[tail] = (short)(N + i); qneg[tail++] = true;
            }
        }
        for (int i = 0; i < nn; i++) { q[tail] = nx[i]; qneg[tail++] = nxneg[i]; }
        nn = 0;
        while (tail - head >= 2) {
            const int k = tail - head >= 3 ? 3 : 2;
            // a group is opened right in front of the cell that takes its parity: its carry goes to the next
            // weight with the sign of its row
            for (int j = 0; j < k; j++)
                if (qgrp[head + j]) {
                    const short in0 = (short)(qgrp[head + j] - 1);
                    NetCell gc = {in0, (short)(in0 + 1), (short)(in0 + 2), -1, -1, BOP_MAJ_NC, (short)w, true};
                    gc.s = (short)p.nwires++;
                    gc.cy = (short)p.nwires++;
                    nx[nn] = gc.cy; nxneg[nn++] = qneg[head + j];
                    p.nops++;
                    q[head + j] = gc.s; qgrp[head + j] = 0;
                    p.cell[p.ncell++] = gc;
                }
            // the positive inputs first
            short in[3] = {-1, -1, -1};
            int np = 0, ng = 0;
            for (int j = 0; j < k; j++) if (!qneg[head + j]) in[np++] = q[head + j];
            for (int j = 0; j < k; j++) if (qneg[head + j]) in[np + ng++] = q[head + j];
            head += k;
            NetCell c = {in[0], in[1], in[2], (short)p.nwires++, -1, 0, (short)w};
            bool sneg = false, cneg = false;
            if (k == 3) {
                sneg = ng & 1; cneg = ng >= 2;
                c.imm = ng == 1 ? BOP_MAJ_NC : ng == 2 ? BOP_BORROW : BOP_MAJ;
            } else {
                // + +: a & b;   + -: -(~a & b);   - -: -(a & b)
                sneg = ng == 2; cneg = ng >= 1;
                c.imm = ng == 1 ? BOP_ANDN : 0;
            }
            p.nops++;
            if (!top) {
                c.cy = (short)p.nwires++;
                nx[nn] = c.cy; nxneg[nn++] = cneg;
                p.nops++;
            }
            q[--head] = c.s; qneg[head] = sneg;
            p.cell[p.ncell++] = c;
        }
        p.out[w] = q[head];
        if (qneg[head] && !top) { nx[nn] = q[head]; nxneg[nn++] = true; }   // -s = s - 2s
    }
    // Order of issue: of the cells whose inputs are there, the one of the HIGHEST weight first, so
    // that carries are used up as they come and few wires are alive at a time.  A cell then reads
    // at the earliest the carry of the cell just before it (IT operations back) or that cell's sum
    // (2 IT operations back): net_min_distance.
    bool made[NetPlan<N, SB>::NIN + 2 * NetPlan<N, SB>::MAXC] = {};
    for (int i = 0; i < NetPlan<N, SB>::NIN; i++) made[i] = true;
    NetCell order[NetPlan<N, SB>::MAXC] = {};
    bool done[NetPlan<N, SB>::MAXC] = {};
    for (int n = 0; n < p.ncell; n++) {
        int pick = -1;
        for (int i = 0; i < p.ncell; i++) {
            const NetCell &c = p.cell[i];
            if (done[i] || !made[c.a] || !made[c.b] || (c.c >= 0 && !made[c.c])) continue;
            if (pick < 0 || c.w > p.cell[pick].w) pick = i;
        }
        done[pick] = true;
        order[n] = p.cell[pick];
        made[order[n].s] = true;
        if (order[n].cy >= 0) made[order[n].cy] = true;
    }
    for (int n = 0; n < p.ncell; n++) p.cell[n] = order[n];
    return p;
}

// the plan of a window, made once; the functions below take a copy of it as a constant of their own
template <int N, int SB, bool GR = false>
struct NetPlanOf { static constexpr NetPlan<N, SB> value = net_make_plan<N, SB, GR>(); };

// the shortest distance, in operations of one item's instruction stream of IT items side by
// side, between an operation and the operation that made one of its inputs
template <int N, int SB, bool GR = false>
constexpr int net_min_distance(int it)
{
    const NetPlan<N, SB> p = NetPlanOf<N, SB, GR>::value;
    int pos[NetPlan<N, SB>::NIN + 2 * NetPlan<N, SB>::MAXC] = {};
    for (int i = 0; i < NetPlan<N, SB>::NIN; i++) pos[i] = -(1 << 20);
    int at = 0, best = 1 << 20;
    for (int n = 0; n < p.ncell; n++) {
        const NetCell &c = p.cell[n];
        const short in[3] = {c.a, c.b, c.c};
        for (int j = 0; j < 3; j++)
            if (in[j] >= 0 && at - pos[in[j]] < best) best = at - pos[in[j]];
        pos[c.s] = at;
        if (!c.grp) at += it;       // (a group's parity is there before its carries are issued)
        if (c.cy >= 0) { pos[c.cy] = at; at += it; }
    }
    return best;
}

// operations of the network per item (the mismatch bits themselves not counted) ...
template <int N, bool GR = false>
constexpr int net_ops() { return net_make_plan<N, bits_for(N * N), GR>().nops; }
// ... and of the separate forms: two carry-save trees N -> HB planes, the HB-plane two's
// complement difference, the ripple add of its sign extension into the SB planes
constexpr int net_ops_count_tree(int n)
{
    int ops = 0, m = n;
    for (int w = 0; w < bits_for(n); w++) {
        int carries = 0;
        while (m >= 3) { ops += 2; m -= 2; carries++; }
        if (m == 2) { ops += 2; m = 1; carries++; }
        m = carries;
    }
    return ops;
}
constexpr int net_ops_addsub(int n)
{
    const int hb = bits_for(n), sb = bits_for(n * n);
    int ops = 2 + 2 * (hb - 1) + 2;
    for (int k = 1; k < sb; k++) ops += k + 1 < sb ? 2 : 1;
    return ops;
}
constexpr int net_ops_separate(int n) { return 2 * net_ops_count_tree(n) + net_ops_addsub(n); }

// ---------------------------------------------------------------------------
// the network itself: S[dd0 + it] += sum_i xin(it, i) - sum_i xin(it, N + i), i < N, for
// it < IT side by side.  Inputs are made when first used.  Every dependency has a distance
// of at least IT operations: the sums of a cell for all items, then its carries.  Grouped: xin(it, 3g + 2)
// and xin(it, N + 3g + 2) are the parities of the groups, every other input is a mismatch bit as before.
// ---------------------------------------------------------------------------
template <int N, int SB, int IT, int DS, int NW, int ID, typename XF>
SM_NET_FN u32 net_wire(const u32 (&S)[DS][SB], int dd0, XF &xin, const u32 (&wr)[IT][NW], int it)
{
    if constexpr (ID < 2 * N) return xin(it, ID);
    else if constexpr (ID < 2 * N + SB) return S[dd0 + it][ID - 2 * N];
    else return wr[it][ID - 2 * N - SB];
}

template <int N, int SB, int IT, int DS, bool GR, int C, int NW, typename XF>
SM_NET_FN void net_cells(u32 (&S)[DS][SB], int dd0, XF &xin, u32 (&wr)[IT][NW])
{
    constexpr NetPlan<N, SB> P = NetPlanOf<N, SB, GR>::value;
    if constexpr (C < P.ncell) {
        constexpr NetCell cl = P.cell[C];
        constexpr int NIN = 2 * N + SB;
        constexpr bool full = cl.c >= 0;
        u32 a[IT], b[IT], c[IT];
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) {
            a[it] = net_wire<N, SB, IT, DS, NW, cl.a>(S, dd0, xin, wr, it);
            b[it] = net_wire<N, SB, IT, DS, NW, cl.b>(S, dd0, xin, wr, it);
            if constexpr (full) c[it] = net_wire<N, SB, IT, DS, NW, cl.c>(S, dd0, xin, wr, it);
            else c[it] = 0u;
        }
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) {
            if constexpr (cl.grp) wr[it][cl.s - NIN] = c[it];
            else {
                if constexpr (full) wr[it][cl.s - NIN] = bop<BOP_XOR3>(a[it], b[it], c[it]);
                else wr[it][cl.s - NIN] = a[it] ^ b[it];
                SM_PIN();
            }
        }
        if constexpr (cl.cy >= 0) {
SM_NET_UNROLL
            for (int it = 0; it < IT; it++) {
                if constexpr (full || cl.imm != 0) wr[it][cl.cy - NIN] = bop<cl.imm>(a[it], b[it], c[it]);
                else wr[it][cl.cy - NIN] = a[it] & b[it];
                SM_PIN();
            }
        }
        SM_SYNC();
        net_cells<N, SB, IT, DS, GR, C + 1, NW>(S, dd0, xin, wr);
    }
}

template <int N, int SB, bool GR = false>
constexpr bool net_planes_from_cells()
{
    constexpr NetPlan<N, SB> P = NetPlanOf<N, SB, GR>::value;
    for (int k = 0; k < SB; k++)
        if (P.out[k] < 2 * N + SB) return false;
    return true;
}

template <int N, int SB, int IT, int DS, bool GR = false, typename XF>
SM_NET_FN void network_lockstep(u32 (&S)[DS][SB], int dd0, XF xin)
{
    constexpr NetPlan<N, SB> P = NetPlanOf<N, SB, GR>::value;
    constexpr int NIN = 2 * N + SB, NW = P.nwires - NIN;
    static_assert(net_planes_from_cells<N, SB, GR>(), "every plane of S' comes out of a cell");
    static_assert(net_min_distance<N, SB, GR>(IT) >= IT, "a cell reads a result made fewer than IT operations before");
    u32 wr[IT][NW];
    net_cells<N, SB, IT, DS, GR, 0, NW>(S, dd0, xin, wr);
SM_NET_UNROLL
    for (int k = 0; k < SB; k++)
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) S[dd0 + it][k] = wr[it][P.out[k] - NIN];
}

// ---------------------------------------------------------------------------
// The counter of a two-wave workgroup's shared warm-up rows (sm_match_bs_kernel.h, WT): NI one-bit inputs -- the
// mismatch bits of HALF window rows of one shift -- to their count on TB = bits_for(NI) planes, in ONE carry-save
// counter.  The sums are zero before the warm-up, so the planes of the count ARE the planes of S: nothing is added
// to anything.  Wired like the row network: every weight is a CHAIN (a cell takes the sum of the cell before it
// and two fresh wires), the cells are issued highest weight first, so one partial sum per weight and a few
// carries are alive per item and four items fit the registers side by side.  All wires are positive.  The top
// plane makes no carries: the count is known to be < 2^TB.
// ---------------------------------------------------------------------------
struct CountCell { short a, b, c, s, cy, w; };       // inputs (c < 0: half adder), sum, carry (< 0: not made), weight

// wire numbers: [0, NI) the inputs, from NI on the outputs of the cells in the order they are made
template <int NI, int TB>
struct CountPlan {
    static constexpr int MAXC = NI + TB;            // a full adder removes a wire; half adders: one per weight
    CountCell cell[MAXC] = {};
    int ncell = 0;
    int nwires = NI;
    int nops = 0;
    short out[TB] = {};         // the wire that is plane k of the count (< 0: the plane is zero)
};

template <int NI, int TB>
constexpr CountPlan<NI, TB> count_make_plan()
{
    static_assert(NI >= 3 && (1 << TB) > NI, "planes of the count");
    CountPlan<NI, TB> p;
    short q[2 * NI + 2 * TB] = {}, nx[NI + TB] = {};
    int head = 0, tail = 0, nn = 0;
    for (int w = 0; w < TB; w++) {
        const bool top = w == TB - 1;
        head = 0; tail = 0;
        if (w == 0)
            for (int i = 0; i < NI; i++) q[tail++] = (short)i;
        for (int i = 0; i < nn; i++) q[tail++] = nx[i];
        nn = 0;
        while (tail - head >= 2) {
            const int k = tail - head >= 3 ? 3 : 2;
            CountCell c = {q[head], q[head + 1], (short)(k == 3 ? q[head + 2] : -1), (short)p.nwires++, -1, (short)w};
            head += k;
            p.nops++;
            if (!top) {
                c.cy = (short)p.nwires++;
                nx[nn++] = c.cy;
                p.nops++;
            }
            q[--head] = c.s;
            p.cell[p.ncell++] = c;
        }
        p.out[w] = tail > head ? q[head] : (short)-1;
    }
    // order of issue: of the cells whose inputs are there, the one of the highest weight first (as net_make_plan)
    bool made[NI + 2 * CountPlan<NI, TB>::MAXC] = {};
    for (int i = 0; i < NI; i++) made[i] = true;
    CountCell order[CountPlan<NI, TB>::MAXC] = {};
    bool done[CountPlan<NI, TB>::MAXC] = {};
    for (int n = 0; n < p.ncell; n++) {
        int pick = -1;
        for (int i = 0; i < p.ncell; i++) {
            const CountCell &c = p.cell[i];
            if (done[i] || !made[c.a] || !made[c.b] || (c.c >= 0 && !made[c.c])) continue;
            if (pick < 0 || c.w > p.cell[pick].w) pick = i;
        }
        done[pick] = true;
        order[n] = p.cell[pick];
        made[order[n].s] = true;
        if (order[n].cy >= 0) made[order[n].cy] = true;
    }
    for (int n = 0; n < p.ncell; n++) p.cell[n] = order[n];
    return p;
}

template <int NI, int TB>
struct CountPlanOf { static constexpr CountPlan<NI, TB> value = count_make_plan<NI, TB>(); };

// the shortest distance, in operations of one item's instruction stream of IT items side by side, between a
// cell's operation and the operation that made one of its inputs (inputs of the counter: made right in front
// of the cell, all items' before the first sum -- at least IT operations before their use)
template <int NI, int TB>
constexpr int count_min_distance(int it)
{
    const CountPlan<NI, TB> p = CountPlanOf<NI, TB>::value;
    int pos[NI + 2 * CountPlan<NI, TB>::MAXC] = {};
    for (int i = 0; i < NI; i++) pos[i] = -(1 << 20);
    int at = 0, best = 1 << 20;
    for (int n = 0; n < p.ncell; n++) {
        const CountCell &c = p.cell[n];
        const short in[3] = {c.a, c.b, c.c};
        for (int j = 0; j < 3; j++)
            if (in[j] >= 0 && at - pos[in[j]] < best) best = at - pos[in[j]];
        pos[c.s] = at;
        at += it;
        if (c.cy >= 0) { pos[c.cy] = at; at += it; }
    }
    return best;
}

// Operations per shift of the shared warm-up rows of an N x N window, the mismatch bits included: in one counter
// (N / 2 * N bits and the cells of the plan) and row by row (per row N bits, a tree N -> HB planes and the ripple
// add of its count into the SB sum planes: 2 for plane 0, a carry and a plane each above, no carry out of the top)
constexpr int warm_ops_tree(int n, int cells_ops) { return n / 2 * n + cells_ops; }
template <int N>
constexpr int warm_ops_tree() { return warm_ops_tree(N, count_make_plan<N / 2 * N, bits_for(N / 2 * N)>().nops); }
constexpr int warm_ops_rows(int n) { return n / 2 * (n + net_ops_count_tree(n) + 2 * bits_for(n * n) - 1); }

template <int NI, int IT, int NW, int ID, typename XF>
SM_NET_FN u32 count_wire(XF &xin, const u32 (&wr)[IT][NW], int it)
{
    if constexpr (ID < NI) return xin(it, ID);
    else return wr[it][ID - NI];
}

template <int NI, int TB, int IT, int C, int NW, typename XF>
SM_NET_FN void count_cells(XF &xin, u32 (&wr)[IT][NW])
{
    constexpr CountPlan<NI, TB> P = CountPlanOf<NI, TB>::value;
    if constexpr (C < P.ncell) {
        constexpr CountCell cl = P.cell[C];
        constexpr bool full = cl.c >= 0;
        u32 a[IT], b[IT], c[IT];
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) {
            a[it] = count_wire<NI, IT, NW, cl.a>(xin, wr, it);
            b[it] = count_wire<NI, IT, NW, cl.b>(xin, wr, it);
            if constexpr (full) c[it] = count_wire<NI, IT, NW, cl.c>(xin, wr, it);
            else c[it] = 0u;
        }
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) {
            if constexpr (full) wr[it][cl.s - NI] = bop<BOP_XOR3>(a[it], b[it], c[it]);
            else wr[it][cl.s - NI] = a[it] ^ b[it];
            SM_PIN();
        }
        if constexpr (cl.cy >= 0) {
SM_NET_UNROLL
            for (int it = 0; it < IT; it++) {
                if constexpr (full) wr[it][cl.cy - NI] = bop<BOP_MAJ>(a[it], b[it], c[it]);
                else wr[it][cl.cy - NI] = a[it] & b[it];
                SM_PIN();
            }
        }
        SM_SYNC();
        count_cells<NI, TB, IT, C + 1, NW>(xin, wr);
    }
}

template <int NI, int TB, int IT, int K, int NW>
SM_NET_FN void count_planes(u32 (&h)[IT][TB], const u32 (&wr)[IT][NW])
{
    if constexpr (K < TB) {
        constexpr CountPlan<NI, TB> P = CountPlanOf<NI, TB>::value;
SM_NET_UNROLL
        for (int it = 0; it < IT; it++) {
            if constexpr (P.out[K] >= NI) h[it][K] = wr[it][P.out[K] - NI];
            else h[it][K] = 0u;
        }
        count_planes<NI, TB, IT, K + 1, NW>(h, wr);
    }
}

// h[it] = the count of xin(it, i), i < NI, for it < IT side by side; inputs are made when first used, in the
// order of their numbers
template <int NI, int TB, int IT, typename XF>
SM_NET_FN void count_chain_lockstep(XF xin, u32 (&h)[IT][TB])
{
    constexpr CountPlan<NI, TB> P = CountPlanOf<NI, TB>::value;
    constexpr int NW = P.nwires - NI;
    static_assert(count_min_distance<NI, TB>(IT) >= IT, "a cell reads a result made fewer than IT operations before");
    u32 wr[IT][NW];
    count_cells<NI, TB, IT, 0, NW>(xin, wr);
    count_planes<NI, TB, IT, 0, NW>(h, wr);
}
