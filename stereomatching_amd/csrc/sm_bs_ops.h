// sm_bs_ops.h -- what the bit-sliced match kernel (sm_match_bs_kernel.h) and its row-step
// network (sm_bs_network.h, also built for the host) share: the v_bitop3 immediates and the
// number of planes of a count.  bop<IMM>(a, b, c) is bit (a<<2|b<<1|c) of IMM.
#pragma once

#define BOP_XOR3 0x96      // a ^ b ^ c
#define BOP_MAJ 0xE8       // majority(a, b, c)
#define BOP_MAJ_NC 0xD4    // majority(a, b, ~c): carry out of a + b - c
#define BOP_BORROW 0x8E    // majority(~a, b, c): borrow out of a - b - c
#define BOP_SEL 0xCA       // a ? b : c
#define BOP_XOR_AND 0x28   // (a ^ b) & c
#define BOP_UPD 0x41       // ~(a ^ b) & ~c
#define BOP_ANDN 0x0C      // ~a & b
#define BOP_ORN 0xCF       // ~a | b   (a ? b : all ones)
#define BOP_XNOR 0xC3      // ~(a ^ b)            (c ignored)

constexpr int bits_for(int v) { int b = 0; while ((1 << b) <= v) b++; return b; }   // v < 2^b
