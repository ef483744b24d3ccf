// Estimator::PlanSamples / ScoreSelect / ScoreCountAbove with scoreDilate, and Estimator::ScoreWindow, from the C++ host.
// A batch of 6 samples per pixel, then:
//   - a plan with scoreDilate = 0, a select and a count of the same statistics: one score image, as before this argument existed;
//   - a plan with scoreDilate = `dilate`: its counts are dumped, sum to the budget and differ from the pointwise plan's; the raw
//     score image is scored again by the plan (it always is) but not by the dilated select and count behind it;
//   - the dilated select's classes equal the dilated plan's, its maximum equals the pointwise maximum, its minimum is not below;
//   - Estimator::ScoreWindow on a caller's image (the opening, MIN then MAX with radius 2), dumped; out over in is refused.
// Dumped for tests/test_score_window_gpu.py, which plans through the Python entries on the same statistics and restates the window:
//   <prefix>.n.i32  <prefix>.film_mean.f32  <prefix>.film_m2.f32   the radiance statistics the scores were made from
//   <prefix>.counts0.i32  <prefix>.counts.i32                       the pointwise and the dilated plan
//   <prefix>.own.f32  <prefix>.eroded.f32  <prefix>.opened.f32      the caller's image and what ScoreWindow made of it
//   test_score_window width height dilate prefix    prints "plan: ..." lines and "score window ok", exits 0; or names the difference
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "statmc_denoiser.hpp"

using namespace statmc;

namespace {

uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
// sample s of pixel (x, y), channel c of stat type `type`: radiance whose spread grows across the film, with rare bright samples
float sampleOf(int type, int x, int y, int s, int c, int width) {
    const uint32_t h = mix32((uint32_t)(y * width + x) * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    if (type != 0) return (float)(h >> 21) * (1.f / 2048.f);
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    return 0.5f + (0.02f + (float)x / (float)width) * (u * u) * ((h & 31u) == 0 ? 20.f : 1.f);
}

struct Film {
    Buffer film;
    BufferRegistry reg;
    Estimator est;
    Film(int w, int h, const StatTypeConfigs &cfgs)
        : film("film", HostImage(h, w, F32C3)), reg(film), est(film, cfgs, 10.f, 20, /*denoiseFilm=*/true, /*acrr=*/false, /*smis=*/false, reg) {
        est.AllocateBuffers(reg);
    }
};

struct DeviceArray {
    void *ptr = nullptr;
    explicit DeviceArray(size_t bytes) { check(statmc_malloc(&ptr, bytes)); }
    DeviceArray(const void *host, size_t bytes, void *stream) {
        check(statmc_malloc(&ptr, bytes));
        check(statmc_upload(ptr, host, bytes, stream));
    }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
};

void dump(const std::string &path, const void *data, size_t bytes) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, bytes, f) != bytes) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

// [S][H][W][3] arenas of the three types, samples s0 .. s0 + S - 1
void accumulate(Estimator &est, int W, int H, int s0, int S) {
    std::vector<float> arena[3];
    for (int i = 0; i < 3; i++)
        for (int s = s0; s < s0 + S; s++)
            for (int k = 0; k < W * H; k++)
                for (int c = 0; c < 3; c++) arena[i].push_back(sampleOf(i, k % W, k / W, s, c, W));
    void *st = est.DeviceStream();
    DeviceArray d0(arena[0].data(), arena[0].size() * sizeof(float), st), d1(arena[1].data(), arena[1].size() * sizeof(float), st),
        d2(arena[2].data(), arena[2].size() * sizeof(float), st);
    est.AccumulateFilm(S, {{0, 0, d0.ptr, STATMC_SAMPLES_F32}, {1, 0, d1.ptr, STATMC_SAMPLES_F32}, {2, 0, d2.ptr, STATMC_SAMPLES_F32}});
    check(statmc_synchronize(st));   // before the arrays are freed
}

statmc_select_result fetch(Estimator &est, const statmc_select_result *d) {
    statmc_select_result r;
    check(statmc_download(&r, d, sizeof(r), est.DeviceStream()));
    est.Synchronize();
    return r;
}

std::vector<int32_t> countsOf(Estimator &est, const Estimator::SamplePlan &plan, int64_t npx) {
    std::vector<int32_t> c((size_t)npx);
    check(statmc_download(c.data(), plan.d_counts, (size_t)npx * 4, est.DeviceStream()));
    est.Synchronize();
    return c;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) {
        std::printf("usage: %s width height dilate prefix\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), DILATE = std::atoi(argv[3]), FIRST = 6;
    const std::string prefix = argv[4];
    const int64_t npx = (int64_t)W * H, budget = npx * 4;
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        Film f(W, H, makeStatTypeConfigs(p));
        Estimator &est = f.est;
        est.EnableDeviceAccumulation((size_t)64 << 20);
        accumulate(est, W, H, 0, FIRST);
        est.DownloadStatistics();
        est.Synchronize();
        dump(prefix + ".n.i32", est.nBuffers[0][0].mat.ptr(), (size_t)npx * 4);
        dump(prefix + ".film_mean.f32", est.filmBuffers[0][0].mat.ptr(), (size_t)npx * 12);
        dump(prefix + ".film_m2.f32", est.filmM2Buffers[0][0].mat.ptr(), (size_t)npx * 12);

        // scoreDilate = 0, given or left out: one score image serves the plan, the select and the counts, as before
        const size_t images0 = est.ScoreImagesComputed();
        const Estimator::SamplePlan plan0 = est.PlanSamples(0, 0, budget, 1, 8, STATMC_SCORE_RELATIVE, 1e-3f, 0);
        const std::vector<int32_t> counts0 = countsOf(est, plan0, npx);
        const std::vector<int64_t> ranks = {0, npx - 1};
        const statmc_select_result sel0 = fetch(est, est.ScoreSelect(0, 0, ranks));
        int64_t above0[1];
        check(statmc_download(above0, est.ScoreCountAbove(0, 0, {0.f}, STATMC_SCORE_RELATIVE, 1e-3f, 0), sizeof(above0), est.DeviceStream()));
        est.Synchronize();
        if (est.ScoreImagesComputed() != images0 + 1) {
            std::printf("MISMATCH %zu score images computed for one plan, one select and one count with scoreDilate 0\n",
                        est.ScoreImagesComputed() - images0);
            return 1;
        }
        dump(prefix + ".counts0.i32", counts0.data(), (size_t)npx * 4);
        std::printf("plan: dilate 0 total %" PRId64 " status %d level 0x%08x\n", plan0.result.total, (int)plan0.result.status, (unsigned)plan0.result.level_bits);

        // scoreDilate > 0: the plan scores again (it always does); the dilated select and count behind it reuse that raw image
        const Estimator::SamplePlan plan = est.PlanSamples(0, 0, budget, 1, 8, STATMC_SCORE_RELATIVE, 1e-3f, DILATE);
        const std::vector<int32_t> counts = countsOf(est, plan, npx);
        const statmc_select_result sel = fetch(est, est.ScoreSelect(0, 0, ranks, STATMC_SCORE_RELATIVE, 1e-3f, DILATE));
        int64_t above[1];
        check(statmc_download(above, est.ScoreCountAbove(0, 0, {0.f}, STATMC_SCORE_RELATIVE, 1e-3f, DILATE), sizeof(above), est.DeviceStream()));
        est.Synchronize();
        if (est.ScoreImagesComputed() != images0 + 2) {
            std::printf("MISMATCH %zu score images computed in all: the windowed image must not touch the raw image's reuse\n",
                        est.ScoreImagesComputed() - images0);
            return 1;
        }
        dump(prefix + ".counts.i32", counts.data(), (size_t)npx * 4);
        std::printf("plan: dilate %d total %" PRId64 " status %d level 0x%08x\n", DILATE, plan.result.total, (int)plan.result.status, (unsigned)plan.result.level_bits);
        int64_t sum = 0;
        for (int32_t c : counts) sum += c;
        if (plan.result.status != 0 || plan.result.total != budget || sum != budget || plan0.result.total != budget) {
            std::printf("MISMATCH the dilated plan spends %" PRId64 " (counts %" PRId64 ") of %" PRId64 "\n", plan.result.total, sum, budget);
            return 1;
        }
        if (DILATE > 0 && counts == counts0) {
            std::printf("MISMATCH the dilated plan equals the pointwise plan\n");
            return 1;
        }
        if (sel.n_live != plan.result.n_live || sel.n_saturated != plan.result.n_saturated) {
            std::printf("MISMATCH the dilated select's classes %" PRId64 " / %" PRId64 " differ from the dilated plan's %d / %d\n", sel.n_live, sel.n_saturated,
                        (int)plan.result.n_live, (int)plan.result.n_saturated);
            return 1;
        }
        if (sel.value_bits[1] != sel0.value_bits[1] || sel.value_bits[0] < sel0.value_bits[0] || above[0] < above0[0]) {
            std::printf("MISMATCH a dilation keeps the maximum and lowers neither the minimum nor a count above a threshold\n");
            return 1;
        }
        // the pointwise select again: the raw image is still the one held, and still gives the first answer
        const statmc_select_result again = fetch(est, est.ScoreSelect(0, 0, ranks));
        if (est.ScoreImagesComputed() != images0 + 2 || std::memcmp(&again, &sel0, sizeof(sel0)) != 0) {
            std::printf("MISMATCH the pointwise select behind a dilated one scored again or differs\n");
            return 1;
        }
        try {
            est.PlanSamples(0, 0, budget, 1, 8, STATMC_SCORE_RELATIVE, 1e-3f, STATMC_SCORE_WINDOW_MAX_RADIUS + 1);
            std::printf("MISMATCH scoreDilate 33 was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }

        // Estimator::ScoreWindow on a caller's image: spikes on every 53rd pixel of a slope; MIN, then MAX of that (the opening)
        std::vector<float> own((size_t)npx);
        for (int64_t k = 0; k < npx; k++) own[(size_t)k] = k % 53 == 0 ? 1e6f : 1.f + (float)(k % W) / (float)W;
        DeviceArray d_own(own.data(), own.size() * sizeof(float), est.DeviceStream()), d_eroded((size_t)npx * 4), d_opened((size_t)npx * 4);
        est.ScoreWindow(static_cast<const float *>(d_own.ptr), STATMC_SCORE_WINDOW_MIN, 2, static_cast<float *>(d_eroded.ptr));
        est.ScoreWindow(static_cast<const float *>(d_eroded.ptr), STATMC_SCORE_WINDOW_MAX, 2, static_cast<float *>(d_opened.ptr));
        std::vector<float> eroded((size_t)npx), opened((size_t)npx);
        check(statmc_download(eroded.data(), d_eroded.ptr, (size_t)npx * 4, est.DeviceStream()));
        check(statmc_download(opened.data(), d_opened.ptr, (size_t)npx * 4, est.DeviceStream()));
        est.Synchronize();
        dump(prefix + ".own.f32", own.data(), (size_t)npx * 4);
        dump(prefix + ".eroded.f32", eroded.data(), (size_t)npx * 4);
        dump(prefix + ".opened.f32", opened.data(), (size_t)npx * 4);
        for (int64_t k = 0; k < npx; k++)
            if (!(opened[(size_t)k] <= own[(size_t)k]) || opened[(size_t)k] >= 1e6f) {
                std::printf("MISMATCH the opening left a spike or rose above the image at pixel %" PRId64 "\n", k);
                return 1;
            }
        try {
            est.ScoreWindow(static_cast<const float *>(d_own.ptr), STATMC_SCORE_WINDOW_MAX, 1, static_cast<float *>(d_own.ptr));
            std::printf("MISMATCH ScoreWindow in place was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        std::printf("score window ok: %dx%d, dilate %d\n", W, H, DILATE);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
