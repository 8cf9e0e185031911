// sm_geom.h -- the launch geometries the planners fill and the kernels take as arguments, and the constants both
// sides share.  No HIP header: sm_plan_model.h (the planners, plain C++17) needs nothing else of the library.
#pragma once

enum { SM_KERNEL_A = 0, SM_KERNEL_B = 1, SM_KERNEL_C = 2, SM_KERNEL_GENERIC = 3, SM_KERNEL_BS = 4 };

#define SM_DSET 16   // shifts per lane in the tiled kernels
#define SM_P 8       // pixels per lane
#define SM_PADT 32   // left pad of a tile's LDS rows, in pixels
#define SM_KEY_DBITS 10  // low bits of the winner key hold the shift

struct MatchGeom {
    int w, h;            // image size
    int D;               // number of shifts
    int n, half;         // window side (odd) and its half
    int ext_words;       // u32 words per ext row
    int ext_rows;        // ext rows per image
    long long ext_image_words;  // ext_words * ext_rows
    int pad_l;           // pixels of left pad in the ext image (multiple of 32)
    // tiled kernels only
    int tile_h;          // output rows per workgroup
    int tw;              // output columns per workgroup (= 8 * runs)
    int runs;            // pixel runs (of 8) per workgroup
    int ds;              // shifts per lane (16; 8 or 16 in the bit-sliced kernel)
    int nl, log2nl;      // lanes that split the shift range of one run
    int threads;         // runs * nl
    int plw, prw;        // words per staged LDS row, left / right
    int nsr;             // staged rows = tile_h + n - 1
    int tiles_x, tiles_y;
    int vec_ok;          // rows are 16-byte aligned -> int4 stores
    int lds_bytes;
    int cap2;            // bit-sliced kernel: launch the two-waves-per-SIMD variant
    int duo;             // bit-sliced kernel: two-wave workgroups of 2 * tile_h rows (shared warm-up)
    int unused[4];       // (where the retired priority fields were: the kernel arguments 16 bytes shorter measured
                         //  2 % slower in the C1 step, edges + match, same device; no kernel reads these words)
    int xmerge;          // bit-sliced kernel: the shift lanes of a word are merged through LDS every 4 rows (nl >= 4)
    int xm_off;          // ... word offset in LDS where the exchange slots of a two-wave workgroup meet and the
                         //     merge buffers lie (wave 0's from here up, wave 1's from here down; a lone wave's from here up)
    int xm_words;        // ... words of one wave's merge buffer
    int web_bytes;       // bytes per element of the web map of THIS launch: 4 (int32), 2, 1
    // ext words per row that can reach a valid output pixel (left image: columns up to W - 1 + half;
    // right: + D - 1 more); the edge kernels compute no others (the tile round-up stays zero)
    int edge_words_l, edge_words_r;
};

// the SAD / SSD cost mode's fast kernels (sm_cost_pc.hip, sm_cost_qs.hip, sm_cost_mfma.hip)
struct SadGeom {
    int w, h, D;
    int ghost;
    int tile_h, tw;          // output rows / columns per (one-wave) workgroup
    int nl, log2nl;          // lanes that split the shift range of one pixel group
    int nql, px;             // shift quads and pixels per lane (the kernel's template arguments)
    int tiles_x, tiles_y;
    int padl;                // bytes left of the tile in a staged row (multiple of 4, >= half + 3)
    int lrow, rrow;          // bytes per staged row, left / right (multiples of 8)
    int nsr;                 // staged rows = tile_h + n - 1
    int q_tail;              // first quad of a lane that may hold shifts >= D
    int q_last;              // last quad in which some lane has a shift < D
    int fast_stage;          // image rows are dword-aligned and w % 4 == 0
    int tbl_pad;             // k_ssd_mfma: dwords between the staged rows and its (16-byte aligned) RR table
    int lds_bytes;
    int waves;               // k_sad_pc: waves per workgroup (they share the staged rows; the other kernels: 1)
};
