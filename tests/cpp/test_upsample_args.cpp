// statmc_upsample_args.h on its own: no library, no device, nothing but include/statmc.h.  Builds one valid call of
// statmc_upsample_filtered -- two argument blocks over made-up image "pointers" (numbers: nothing is read through them) -- and one
// mutation of it per rule of the header, and prints check_upsample_call's verdict for each, and for the valid ones what
// fill_upsample_args made of them.  tests/test_upsample_cpu.py holds the lines against its table of the rules.
//
// Output, one line per call:   <name> : <code> <message>   |   <name> : 0 ok <shift> <wc> <hc> <vec> <p_begin> <p_end> <grid> <roi>
#include <functional>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_upsample_args.h"

namespace {

constexpr int kW = 37, kH = 23, kB = 2, kG = 3;

// Both sides of a call with their tables; the images sit 1 MiB apart from address 16 MiB on, so that none overlaps another.
struct Call {
    statmc_filter_args fine, coarse;
    statmc_image f_mc[kB], f_disc[kB], f_film[kB], f_out[kB], f_g[kG];
    statmc_image c_mc[kB], c_disc[kB], c_out[kB], c_g[kG];
    uint8_t gch[kG], c_gch[kG];
    float dr[kG];
    int k, channels, dof;
    uintptr_t next;

    statmc_image image(int w, int h, int ch) {
        statmc_image im;
        im.data = reinterpret_cast<void *>(next);
        next += 1u << 20;
        im.step = (size_t)w * ch * 4, im.cols = w, im.rows = h;
        return im;
    }

    Call(int k_, int channels_) : k(k_), channels(channels_), dof(STATMC_DOF_PIXEL), next(16u << 20) {
        memset(&fine, 0, sizeof(fine));
        memset(&coarse, 0, sizeof(coarse));
        const int wc = (kW + k - 1) / k, hc = (kH + k - 1) / k;
        const uint8_t g[kG] = {3, 3, 1};
        for (int b = 0; b < kB; b++) {
            f_mc[b] = image(kW, kH, channels), f_disc[b] = image(kW, kH, channels), f_film[b] = image(kW, kH, channels), f_out[b] = image(kW, kH, channels);
            c_mc[b] = image(wc, hc, channels), c_disc[b] = image(wc, hc, channels), c_out[b] = image(wc, hc, channels);
        }
        for (int i = 0; i < kG; i++) gch[i] = c_gch[i] = g[i], dr[i] = -0.5f, f_g[i] = image(kW, kH, g[i]), c_g[i] = image(wc, hc, g[i]);
        fine.n_buffers = coarse.n_buffers = kB;
        fine.width = kW, fine.height = kH, coarse.width = (uint16_t)wc, coarse.height = (uint16_t)hc;
        fine.mean_corr = f_mc, fine.discriminator = f_disc, fine.film = f_film, fine.film_filtered = f_out;
        coarse.mean_corr = c_mc, coarse.discriminator = c_disc, coarse.film_filtered = c_out;
        fine.g_buffers = f_g, fine.g_channel_counts = gch, fine.g_dr_factors = dr, fine.n_g_buffers = kG;
        coarse.g_buffers = c_g, coarse.g_channel_counts = c_gch, coarse.g_dr_factors = dr, coarse.n_g_buffers = kG;
    }
};

int n_calls = 0;

void run(const char *name, int k, int channels, const std::function<void(Call &)> &change, bool null_fine = false, bool null_coarse = false) {
    Call c(k, channels);
    if (change) change(c);
    char why[512] = "";
    const int rc = statmc::check_upsample_call(null_fine ? nullptr : &c.fine, null_coarse ? nullptr : &c.coarse, c.k, c.channels, c.dof,
                                               statmc::UpsampleMsg{why, sizeof(why)});
    n_calls++;
    if (rc != STATMC_OK) {
        printf("%s : %d %s\n", name, rc, why);
        return;
    }
    statmc_filter_spec spec = {};
    spec.border = STATMC_BORDER_CLAMP;
    statmc::UpsampleArgs a;
    statmc::fill_upsample_args(a, &c.fine, &c.coarse, c.k, c.channels, 0, spec);
    printf("%s : 0 ok %d %d %d %d %lld %lld %lld %d,%d,%d,%d\n", name, a.shift, a.wc, a.hc, a.vec, a.p_begin, a.p_end, statmc::upsample_grid(a), a.rx0, a.ry0,
           a.rx1, a.ry1);
}

}  // namespace

int main() {
    run("valid_k2_rgb", 2, 3, nullptr);
    run("valid_k4_rgb", 4, 3, nullptr);
    run("valid_k8_float", 8, 1, nullptr);
    run("valid_roi", 2, 3, [](Call &c) { c.fine.roi_x0 = 3, c.fine.roi_y0 = 5, c.fine.roi_x1 = 30, c.fine.roi_y1 = 9; });
    run("valid_unaligned_plane", 2, 3, [](Call &c) { c.f_g[1].data = static_cast<char *>(c.f_g[1].data) + 4; });
    run("valid_denoise_film_without_film_tables", 2, 3, [](Call &c) {
        c.fine.n_buffers = c.coarse.n_buffers = 1;
        c.fine.denoise_film = c.coarse.denoise_film = 1;
        c.fine.film_buffer = c.f_film[0], c.fine.film_filtered_buffer = c.f_out[0], c.coarse.film_filtered_buffer = c.c_out[0];
        c.fine.film = nullptr, c.fine.film_filtered = nullptr, c.coarse.film_filtered = nullptr;
    });
    run("valid_no_g_buffers", 2, 3, [](Call &c) {
        c.fine.n_g_buffers = c.coarse.n_g_buffers = 0;
        c.fine.g_buffers = c.coarse.g_buffers = nullptr;
    });
    run("null_fine", 2, 3, nullptr, true, false);
    run("null_coarse", 2, 3, nullptr, false, true);
    run("k_3", 3, 3, nullptr);
    run("k_16", 16, 3, nullptr);
    run("k_comes_before_channels", 1, 2, nullptr);
    run("channels_2", 2, 2, nullptr);
    run("empty_fine", 2, 3, [](Call &c) { c.fine.width = 0; });
    run("coarse_size_floor", 2, 3, [](Call &c) { c.coarse.width = kW / 2; });
    run("coarse_height", 4, 3, [](Call &c) { c.coarse.height += 1; });
    run("n_buffers_differ", 2, 3, [](Call &c) { c.coarse.n_buffers = 1; });
    run("n_g_buffers_differ", 2, 3, [](Call &c) { c.coarse.n_g_buffers = 2; });
    run("g_channel_counts_differ", 2, 3, [](Call &c) { c.c_gch[2] = 3; });
    run("null_g_table", 2, 3, [](Call &c) { c.fine.g_dr_factors = nullptr; });
    run("null_coarse_g_table", 2, 3, [](Call &c) { c.coarse.g_buffers = nullptr; });
    run("welch", 2, 3, [](Call &c) { c.dof = STATMC_DOF_WELCH; });
    run("size_comes_before_welch", 2, 3, [](Call &c) { c.dof = STATMC_DOF_WELCH, c.coarse.width += 1; });
    run("packed_fine", 2, 3, [](Call &c) { c.fine.packed_inputs = c.f_mc[0]; });
    run("packed_coarse", 2, 3, [](Call &c) { c.coarse.packed_inputs = c.c_mc[0]; });
    run("three_rgb_g_buffers", 2, 3, [](Call &c) { c.gch[2] = c.c_gch[2] = 3, c.f_g[2].step *= 3, c.c_g[2].step *= 3; });
    run("g_channels_2", 2, 3, [](Call &c) { c.gch[2] = c.c_gch[2] = 2; });
    run("null_mean_corr_table", 2, 3, [](Call &c) { c.fine.mean_corr = nullptr; });
    run("null_coarse_discriminator_table", 2, 3, [](Call &c) { c.coarse.discriminator = nullptr; });
    run("null_film_table", 2, 3, [](Call &c) { c.fine.film = nullptr; });
    run("null_coarse_filtered_table", 2, 3, [](Call &c) { c.coarse.film_filtered = nullptr; });
    run("null_image", 2, 3, [](Call &c) { c.f_disc[1].data = nullptr; });
    run("null_coarse_image", 2, 3, [](Call &c) { c.c_out[0].data = nullptr; });
    run("image_size", 2, 3, [](Call &c) { c.c_mc[1].cols += 1; });
    run("short_pitch", 2, 3, [](Call &c) { c.f_film[0].step -= 4; });
    run("pitched_fine", 2, 3, [](Call &c) { c.f_film[0].step += 64; });
    run("pitched_coarse_g", 2, 3, [](Call &c) { c.c_g[0].step += 16; });
    run("misaligned", 2, 3, [](Call &c) { c.f_mc[0].data = static_cast<char *>(c.f_mc[0].data) + 2; });
    run("roi_outside", 2, 3, [](Call &c) { c.fine.roi_x1 = kW + 1, c.fine.roi_y1 = 4; });
    run("roi_empty", 2, 3, [](Call &c) { c.fine.roi_x0 = 5, c.fine.roi_x1 = 5, c.fine.roi_y1 = 4; });
    run("image_comes_before_roi", 2, 3, [](Call &c) { c.fine.roi_x1 = kW + 1, c.fine.roi_y1 = 4, c.f_mc[0].data = nullptr; });
    run("out_is_colour", 2, 3, [](Call &c) { c.f_out[0].data = c.f_film[0].data; });
    run("out_overlaps_mean_corr_tail", 2, 3, [](Call &c) { c.f_out[1].data = static_cast<char *>(c.f_mc[0].data) + (size_t)kW * kH * 12 - 4; });
    run("out_is_other_out", 2, 3, [](Call &c) { c.f_out[1].data = c.f_out[0].data; });
    run("out_overlaps_coarse_filtered", 2, 3, [](Call &c) { c.c_out[1].data = static_cast<char *>(c.f_out[0].data) + 16; });
    run("out_overlaps_fine_g", 2, 3, [](Call &c) { c.f_g[2].data = static_cast<char *>(c.f_out[0].data) + 64; });
    run("out_overlaps_coarse_g", 2, 3, [](Call &c) { c.c_g[0].data = c.f_out[1].data; });
    run("roi_comes_before_overlap", 2, 3, [](Call &c) { c.f_out[0].data = c.f_film[0].data, c.fine.roi_x0 = -1, c.fine.roi_x1 = 4, c.fine.roi_y1 = 4; });
    return n_calls > 0 ? 0 : 2;
}
