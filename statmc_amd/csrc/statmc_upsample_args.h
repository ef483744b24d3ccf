// statmc_upsample_args.h -- what statmc_upsample_filtered (include/statmc.h) checks and fills on the host, each rule stated once, and
// the argument block its kernel takes (statmc_upsample.hip).  Pure functions of their arguments: no HIP call, no device, no global or
// thread-local state; nothing is read through a pointer but the two argument blocks and their tables (the image pointers are
// compared as numbers).  The verdict is the call's return code -- STATMC_OK, STATMC_ERR_INVALID or STATMC_ERR_UNSUPPORTED -- and the
// caller's buffer names the argument.  Host-only and on its own: tests/cpp/test_upsample_args.cpp compiles this header with nothing
// but include/statmc.h, with and without sanitizers.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/statmc.h"

namespace statmc {

constexpr int kUpsampleBlock = 256;       // 4 waves
constexpr int kUpsampleQuad = 4;          // consecutive fine pixels per lane
constexpr int kUpsampleMaxG = 4;          // the pair-symmetric filter's set: up to two RGB and two one-channel G-buffers

// One buffer of a call as the kernel walks it.  Fine planes are [height][width][channels], coarse ones [hc][wc][channels].
struct UpsampleArgs {
    const float *mean_corr, *disc, *colour;          // fine
    float *out;                                      // the fine filtered image
    const float *c_mean_corr, *c_disc, *c_colour;    // coarse; c_colour: the coarse FILTERED image
    const float *g[kUpsampleMaxG], *c_g[kUpsampleMaxG];
    float dr[kUpsampleMaxG];
    int gc[kUpsampleMaxG];
    int n_g, channels;
    int width, height, wc, hc;
    int shift;                    // log2(2 k): floor_div(t, 2 k) = t >> shift, t mod 2 k = t & (2 k - 1)
    float inv_2k;                 // 1 / (2 k), a power of two
    int rx0, ry0, rx1, ry1;       // the pixels written
    int gate, channel_rule, clamp;
    int vec;                      // every fine plane 16-byte aligned: a lane's full quad moves as dwordx4
    long long p_begin, p_end;     // the flat pixel range the launch covers: the ROI's rows, begun on a quad
};

struct UpsampleMsg { char *buf; size_t len; };   // the caller's buffer
__attribute__((format(printf, 3, 4))) inline int upsample_refuse(UpsampleMsg m, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m.buf, m.len, fmt, ap);
    va_end(ap);
    return code;
}

inline int upsample_coarse(int fine, int k) { return (fine + k - 1) / k; }
inline bool upsample_misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool upsample_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

// an image of a side: data, size, then the row pitch (too short: invalid; longer than a row: a pitched image, unsupported)
inline int upsample_check_image(const statmc_image &im, int w, int h, int ch, const char *side, const char *what, int idx, UpsampleMsg m) {
    if (!im.data) return upsample_refuse(m, STATMC_ERR_INVALID, "%s->%s[%d]: null device pointer", side, what, idx);
    if (im.cols != w || im.rows != h)
        return upsample_refuse(m, STATMC_ERR_INVALID, "%s->%s[%d]: %dx%d image, expected %dx%d", side, what, idx, im.cols, im.rows, w, h);
    const size_t row = (size_t)w * ch * 4;
    if (im.step < row) return upsample_refuse(m, STATMC_ERR_INVALID, "%s->%s[%d]: row pitch %zu is shorter than a row (%zu)", side, what, idx, im.step, row);
    if (im.step != row)
        return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "%s->%s[%d]: row pitch %zu, statmc_upsample_filtered needs packed rows (%zu)", side, what,
                               idx, im.step, row);
    if (upsample_misaligned(im.data, 4)) return upsample_refuse(m, STATMC_ERR_INVALID, "%s->%s[%d] is not 4-byte aligned", side, what, idx);
    return STATMC_OK;
}

inline bool upsample_film_buffer(const statmc_filter_args *a, int b, int channels) { return a->denoise_film && b == 0 && channels == 3; }
inline const statmc_image &upsample_colour(const statmc_filter_args *a, int b, int channels) {
    return upsample_film_buffer(a, b, channels) ? a->film_buffer : a->film[b];
}
inline const statmc_image &upsample_filtered(const statmc_filter_args *a, int b, int channels) {
    return upsample_film_buffer(a, b, channels) ? a->film_filtered_buffer : a->film_filtered[b];
}

// statmc_upsample_filtered, in this order: the argument blocks, k, channels, the two sizes, the counts that must agree, the degrees
// of freedom (`dof`: the current device's statmc_filter_spec.dof), packed inputs, the G-buffer set, NULL tables, every image the call
// touches (fine side, then coarse, per buffer, then the G-buffers), the ROI, the output over an input.
inline int check_upsample_call(const statmc_filter_args *fine, const statmc_filter_args *coarse, int k, int channels, int dof, UpsampleMsg m) {
    if (!fine) return upsample_refuse(m, STATMC_ERR_INVALID, "null fine");
    if (!coarse) return upsample_refuse(m, STATMC_ERR_INVALID, "null coarse");
    if (k != 2 && k != 4 && k != 8) return upsample_refuse(m, STATMC_ERR_INVALID, "k = %d: must be 2, 4 or 8", k);
    if (channels != 1 && channels != 3) return upsample_refuse(m, STATMC_ERR_INVALID, "channels = %d: must be 1 or 3", channels);
    const int W = fine->width, H = fine->height;
    if (W == 0 || H == 0) return upsample_refuse(m, STATMC_ERR_INVALID, "fine: empty image: width and height must be positive");
    const int wc = upsample_coarse(W, k), hc = upsample_coarse(H, k);
    if (coarse->width != wc || coarse->height != hc)
        return upsample_refuse(m, STATMC_ERR_INVALID, "coarse is %dx%d: a %dx%d film pooled by k = %d is %dx%d", (int)coarse->width,
                               (int)coarse->height, W, H, k, wc, hc);
    if (fine->n_buffers > STATMC_MAX_BUFFERS) return upsample_refuse(m, STATMC_ERR_INVALID, "fine->n_buffers > %d", STATMC_MAX_BUFFERS);
    if (fine->n_buffers != coarse->n_buffers)
        return upsample_refuse(m, STATMC_ERR_INVALID, "n_buffers differs: fine %d, coarse %d", (int)fine->n_buffers, (int)coarse->n_buffers);
    if (fine->n_g_buffers != coarse->n_g_buffers)
        return upsample_refuse(m, STATMC_ERR_INVALID, "n_g_buffers differs: fine %zu, coarse %zu", fine->n_g_buffers, coarse->n_g_buffers);
    if (fine->n_g_buffers > STATMC_MAX_GBUFFERS) return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "n_g_buffers > %d", STATMC_MAX_GBUFFERS);
    const int n_b = fine->n_buffers, n_g = (int)fine->n_g_buffers;
    if (n_g && (!fine->g_buffers || !fine->g_channel_counts || !fine->g_dr_factors))
        return upsample_refuse(m, STATMC_ERR_INVALID, "fine: null G-buffer table (g_buffers, g_channel_counts, g_dr_factors)");
    if (n_g && (!coarse->g_buffers || !coarse->g_channel_counts)) return upsample_refuse(m, STATMC_ERR_INVALID, "coarse: null G-buffer table (g_buffers, g_channel_counts)");
    for (int g = 0; g < n_g; g++)
        if (fine->g_channel_counts[g] != coarse->g_channel_counts[g])
            return upsample_refuse(m, STATMC_ERR_INVALID, "g_channel_counts[%d] differs: fine %d, coarse %d", g, (int)fine->g_channel_counts[g],
                                   (int)coarse->g_channel_counts[g]);
    if (dof == STATMC_DOF_WELCH)
        return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "STATMC_DOF_WELCH: the discriminator image holds s^2 / n, not a discriminator");
    if (fine->packed_inputs.data) return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "fine->packed_inputs: block + halo images are not upsampled");
    if (coarse->packed_inputs.data) return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "coarse->packed_inputs: block + halo images are not upsampled");
    int n_rgb = 0, n_sc = 0;
    for (int g = 0; g < n_g; g++) {
        const int gc = fine->g_channel_counts[g];
        if (gc != 1 && gc != 3) return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "g_channel_counts[%d] = %d: 1 or 3", g, gc);
        if ((gc == 3 ? ++n_rgb : ++n_sc) > 2)
            return upsample_refuse(m, STATMC_ERR_UNSUPPORTED, "g_buffers: more than two RGB or two one-channel G-buffers (g_buffers[%d])", g);
    }
    const bool tables_f = upsample_film_buffer(fine, 0, channels) && n_b == 1, tables_c = upsample_film_buffer(coarse, 0, channels) && n_b == 1;
    if (n_b && (!fine->mean_corr || !fine->discriminator)) return upsample_refuse(m, STATMC_ERR_INVALID, "fine: null mean_corr / discriminator table");
    if (n_b && (!coarse->mean_corr || !coarse->discriminator)) return upsample_refuse(m, STATMC_ERR_INVALID, "coarse: null mean_corr / discriminator table");
    if (n_b && !tables_f && (!fine->film || !fine->film_filtered)) return upsample_refuse(m, STATMC_ERR_INVALID, "fine: null film / film_filtered table");
    if (n_b && !tables_c && !coarse->film_filtered) return upsample_refuse(m, STATMC_ERR_INVALID, "coarse: null film_filtered table");
    for (int b = 0; b < n_b; b++) {
        const bool ff = upsample_film_buffer(fine, b, channels), fc = upsample_film_buffer(coarse, b, channels);
        if (int rc = upsample_check_image(fine->mean_corr[b], W, H, channels, "fine", "mean_corr", b, m)) return rc;
        if (int rc = upsample_check_image(fine->discriminator[b], W, H, channels, "fine", "discriminator", b, m)) return rc;
        if (int rc = upsample_check_image(upsample_colour(fine, b, channels), W, H, channels, "fine", ff ? "film_buffer" : "film", b, m)) return rc;
        if (int rc = upsample_check_image(upsample_filtered(fine, b, channels), W, H, channels, "fine", ff ? "film_filtered_buffer" : "film_filtered", b, m))
            return rc;
        if (int rc = upsample_check_image(coarse->mean_corr[b], wc, hc, channels, "coarse", "mean_corr", b, m)) return rc;
        if (int rc = upsample_check_image(coarse->discriminator[b], wc, hc, channels, "coarse", "discriminator", b, m)) return rc;
        if (int rc = upsample_check_image(upsample_filtered(coarse, b, channels), wc, hc, channels, "coarse", fc ? "film_filtered_buffer" : "film_filtered", b, m))
            return rc;
    }
    for (int g = 0; g < n_g; g++) {
        if (int rc = upsample_check_image(fine->g_buffers[g], W, H, fine->g_channel_counts[g], "fine", "g_buffers", g, m)) return rc;
        if (int rc = upsample_check_image(coarse->g_buffers[g], wc, hc, fine->g_channel_counts[g], "coarse", "g_buffers", g, m)) return rc;
    }
    const bool whole = fine->roi_x0 == 0 && fine->roi_y0 == 0 && fine->roi_x1 == 0 && fine->roi_y1 == 0;
    if (!whole && (fine->roi_x0 < 0 || fine->roi_y0 < 0 || fine->roi_x1 > W || fine->roi_y1 > H || fine->roi_x0 >= fine->roi_x1 || fine->roi_y0 >= fine->roi_y1))
        return upsample_refuse(m, STATMC_ERR_INVALID, "fine: roi [%d,%d)x[%d,%d) outside the %dx%d image", fine->roi_x0, fine->roi_x1, fine->roi_y0,
                               fine->roi_y1, W, H);
    const size_t fb = (size_t)W * H * channels * 4, cb = (size_t)wc * hc * channels * 4;
    for (int b = 0; b < n_b; b++) {
        const void *out = upsample_filtered(fine, b, channels).data;
        for (int j = 0; j < n_b; j++) {
            if (upsample_overlap(out, fb, fine->mean_corr[j].data, fb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps fine->mean_corr[%d]", b, j);
            if (upsample_overlap(out, fb, fine->discriminator[j].data, fb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps fine->discriminator[%d]", b, j);
            if (upsample_overlap(out, fb, upsample_colour(fine, j, channels).data, fb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps the fine colour image %d", b, j);
            if (j != b && upsample_overlap(out, fb, upsample_filtered(fine, j, channels).data, fb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps output %d", b, j);
            if (upsample_overlap(out, fb, coarse->mean_corr[j].data, cb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps coarse->mean_corr[%d]", b, j);
            if (upsample_overlap(out, fb, coarse->discriminator[j].data, cb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps coarse->discriminator[%d]", b, j);
            if (upsample_overlap(out, fb, upsample_filtered(coarse, j, channels).data, cb)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps the coarse filtered image %d", b, j);
        }
        for (int g = 0; g < n_g; g++) {
            const size_t gc = fine->g_channel_counts[g];
            if (upsample_overlap(out, fb, fine->g_buffers[g].data, (size_t)W * H * gc * 4)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps fine->g_buffers[%d]", b, g);
            if (upsample_overlap(out, fb, coarse->g_buffers[g].data, (size_t)wc * hc * gc * 4)) return upsample_refuse(m, STATMC_ERR_INVALID, "output %d overlaps coarse->g_buffers[%d]", b, g);
        }
    }
    return STATMC_OK;
}

// The kernel's argument block for buffer b of a call that passed check_upsample_call.
inline void fill_upsample_args(UpsampleArgs &a, const statmc_filter_args *fine, const statmc_filter_args *coarse, int k, int channels, int b,
                               const statmc_filter_spec &spec) {
    a = UpsampleArgs{};
    a.mean_corr = static_cast<const float *>(fine->mean_corr[b].data);
    a.disc = static_cast<const float *>(fine->discriminator[b].data);
    a.colour = static_cast<const float *>(upsample_colour(fine, b, channels).data);
    a.out = static_cast<float *>(upsample_filtered(fine, b, channels).data);
    a.c_mean_corr = static_cast<const float *>(coarse->mean_corr[b].data);
    a.c_disc = static_cast<const float *>(coarse->discriminator[b].data);
    a.c_colour = static_cast<const float *>(upsample_filtered(coarse, b, channels).data);
    a.n_g = (int)fine->n_g_buffers, a.channels = channels;
    a.vec = !upsample_misaligned(a.mean_corr, 16) && !upsample_misaligned(a.disc, 16) && !upsample_misaligned(a.colour, 16) && !upsample_misaligned(a.out, 16);
    for (int g = 0; g < a.n_g; g++) {
        a.g[g] = static_cast<const float *>(fine->g_buffers[g].data);
        a.c_g[g] = static_cast<const float *>(coarse->g_buffers[g].data);
        a.dr[g] = fine->g_dr_factors[g];
        a.gc[g] = fine->g_channel_counts[g];
        a.vec = a.vec && !upsample_misaligned(a.g[g], 16);
    }
    a.width = fine->width, a.height = fine->height;
    a.wc = upsample_coarse(a.width, k), a.hc = upsample_coarse(a.height, k);
    a.shift = k == 2 ? 2 : k == 4 ? 3 : 4;
    a.inv_2k = 1.f / (float)(2 * k);
    const bool whole = fine->roi_x0 == 0 && fine->roi_y0 == 0 && fine->roi_x1 == 0 && fine->roi_y1 == 0;
    a.rx0 = whole ? 0 : fine->roi_x0, a.ry0 = whole ? 0 : fine->roi_y0;
    a.rx1 = whole ? a.width : fine->roi_x1, a.ry1 = whole ? a.height : fine->roi_y1;
    a.gate = spec.gate, a.channel_rule = spec.channel_rule, a.clamp = spec.border == STATMC_BORDER_CLAMP;
    a.p_begin = ((long long)a.ry0 * a.width) & ~(long long)(kUpsampleQuad - 1);
    a.p_end = (long long)a.ry1 * a.width;
}

inline long long upsample_grid(const UpsampleArgs &a) {
    const long long quads = (a.p_end - a.p_begin + kUpsampleQuad - 1) / kUpsampleQuad;
    return (quads + kUpsampleBlock - 1) / kUpsampleBlock;
}

}  // namespace statmc
