/* ref_step3_driver.c -- calls the reference's OWN step-3 functions on a map of
 * our choosing (TEST INFRASTRUCTURE, build container only; see Makefile `ref`).
 *
 * Linked with an unmodified src/stereo.c or src/stereo-ghost.c compiled with
 * -Dmain=ref_main, so the two functions below are the reference's:
 *
 *     i32 *fill_web_holes(i32 *web, int width, int height, int times);
 *     void draw_contour_map(i32 *web, int width, int height, int num_lines, u8 *out);
 *
 *     step3-ref IN OUT
 *
 * IN:  int32 w, h, times, lines, then w*h int32 (the map), little-endian.
 * OUT: the map fill_web_holes RETURNED (w*h int32), written and flushed before
 *      the contour stage, then the contour image (w*h bytes).  A zero contour
 *      interval traps in draw_contour_map (SIGFPE) as it does in the reference
 *      program; OUT then holds the filled map only.
 *
 * Only the pointer fill_web_holes RETURNS is used and freed afterwards: it
 * frees the buffer it does not return. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int32_t *fill_web_holes(int32_t *web, int width, int height, int times);
void draw_contour_map(int32_t *web, int width, int height, int num_lines, uint8_t *out);

static int fail(const char *what)
{
    perror(what);
    return 2;
}

int main(int argc, char *argv[])
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    if (!in) return fail(argv[1]);
    int32_t hdr[4];
    if (fread(hdr, sizeof(int32_t), 4, in) != 4) return fail("header");
    const int w = hdr[0], h = hdr[1], times = hdr[2], lines = hdr[3];
    if (w < 1 || h < 1 || times < 0) {
        fprintf(stderr, "bad header %d %d %d %d\n", w, h, times, lines);
        return 2;
    }
    const size_t n = (size_t)w * h;
    /* exactly n elements: an access outside the map is outside the allocation */
    int32_t *web = malloc(sizeof(int32_t) * n);
    uint8_t *out = malloc(n);
    if (!web || !out) return fail("malloc");
    if (fread(web, sizeof(int32_t), n, in) != n) return fail("map");
    fclose(in);

    web = fill_web_holes(web, w, h, times);

    FILE *o = fopen(argv[2], "wb");
    if (!o) return fail(argv[2]);
    if (fwrite(web, sizeof(int32_t), n, o) != n || fflush(o)) return fail("write map");
    draw_contour_map(web, w, h, lines, out);
    if (fwrite(out, 1, n, o) != n || fclose(o)) return fail("write contour");
    free(web);
    free(out);
    return 0;
}
