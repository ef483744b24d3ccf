// Estimator::PlanToTarget and the trailing scoreOf of PlanSamples / ScoreSelect / ScoreCountAbove, from the C++ host.
// A batch of 6 samples per pixel, then:
//   - reuse and staleness of the score image across scoreOf: a select of the deviation, of the standard error, of the standard error
//     again (reused), of the deviation again (stale: the image held is the standard error's);
//   - the standard error's quantile is below the deviation's, the confidence half-width's above the standard error's;
//   - staleness after statmc_set_significance: a select of the confidence half-width, the level changed, the same select scores
//     again and gives another value; the level set back gives the first value again;
//   - PlanToTarget without a budget: every count in [cMin, cMax], total == the counts' sum, dumped; with a budget of one sample
//     per pixel below its total: the fallback runs, the counts sum to the budget to the sample, the target result is unchanged;
//   - scoreOf = ScoreOfDeviation is refused by PlanToTarget, scoreOf = 3 by all.
// Dumped for tests/test_error_scores_gpu.py, which plans through the Python entries on the same statistics:
//   <prefix>.n.i32  <prefix>.film_mean.f32  <prefix>.film_m2.f32   the radiance statistics the scores were made from
//   <prefix>.counts.i32                                             PlanToTarget's counts (no budget, scoreOf ScoreOfStdErr)
//   test_plan_to_target width height target prefix    prints "target: ..." and "plan to target ok", exits 0; or names the difference
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

// the value of the one rank a select was asked for
float valueOf(Estimator &est, const statmc_select_result *d) {
    statmc_select_result r;
    check(statmc_download(&r, d, sizeof(r), est.DeviceStream()));
    est.Synchronize();
    float v;
    std::memcpy(&v, &r.value_bits[0], sizeof(v));
    return v;
}

std::vector<int32_t> countsOf(Estimator &est, const int32_t *d_counts, int64_t npx) {
    std::vector<int32_t> c((size_t)npx);
    check(statmc_download(c.data(), d_counts, (size_t)npx * 4, est.DeviceStream()));
    est.Synchronize();
    return c;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) {
        std::printf("usage: %s width height target prefix\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), FIRST = 6;
    const float TARGET = std::strtof(argv[3], nullptr);
    const std::string prefix = argv[4];
    const int64_t npx = (int64_t)W * H;
    const int32_t C_MIN = 1, C_MAX = 64;
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

        // ---- reuse and staleness across scoreOf
        const std::vector<int64_t> median = {npx / 2};
        const int REL = STATMC_SCORE_RELATIVE;
        size_t images = est.ScoreImagesComputed();
        auto computed = [&](size_t want, const char *what) {
            const size_t got = est.ScoreImagesComputed() - images;
            images = est.ScoreImagesComputed();
            if (got != want) std::printf("MISMATCH %s: %zu score images computed, expected %zu\n", what, got, want);
            return got == want;
        };
        const float sd = valueOf(est, est.ScoreSelect(0, 0, median));   // the default: the calls made before scoreOf existed
        if (!computed(1, "the first select")) return 1;
        const float sd2 = valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfDeviation));
        if (!computed(0, "the deviation, named") || sd2 != sd) return 1;
        const float se = valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfStdErr));
        if (!computed(1, "the standard error behind the deviation")) return 1;
        int64_t above[1];
        check(statmc_download(above, est.ScoreCountAbove(0, 0, {se}, REL, 1e-3f, 0, Estimator::ScoreOfStdErr), sizeof(above), est.DeviceStream()));
        est.Synchronize();
        if (!computed(0, "the standard error again")) return 1;
        if (above[0] <= 0 || above[0] >= npx) {
            std::printf("MISMATCH %" PRId64 " pixels above the median standard error\n", above[0]);
            return 1;
        }
        const float sd3 = valueOf(est, est.ScoreSelect(0, 0, median));
        if (!computed(1, "the deviation behind the standard error") || sd3 != sd) {
            std::printf("MISMATCH the deviation's median %a after the standard error's, %a before\n", (double)sd3, (double)sd);
            return 1;
        }
        // 6 samples: stderr = sd / sqrt(6) up to roundings, the median's pixel included
        if (!(se > sd * 0.40f && se < sd * 0.42f)) {
            std::printf("MISMATCH median standard error %g is not the median deviation %g over sqrt(6)\n", (double)se, (double)sd);
            return 1;
        }

        // ---- staleness after statmc_set_significance
        // (the Estimator's device is this thread's current one: every call above selected it)
        const int level0 = statmc_get_significance(), level1 = (level0 + 1) % 3;
        const float ci0 = valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfCI));
        if (!computed(1, "the confidence half-width")) return 1;
        valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfCI));
        if (!computed(0, "the confidence half-width again")) return 1;
        check(statmc_set_significance(level1));
        const float ci1 = valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfCI));
        const bool rescored = computed(1, "the confidence half-width at another significance level");
        check(statmc_set_significance(level0));
        if (!rescored) return 1;
        const float ci2 = valueOf(est, est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, Estimator::ScoreOfCI));
        if (!computed(1, "the confidence half-width at the first level again")) return 1;
        if (ci1 == ci0 || ci2 != ci0 || !(ci0 > se) || !(ci1 > se)) {
            std::printf("MISMATCH half-widths %g, %g, %g at levels %d, %d, %d; standard error %g\n", (double)ci0, (double)ci1, (double)ci2, level0, level1,
                        level0, (double)se);
            return 1;
        }

        // ---- PlanToTarget, no budget
        const Estimator::TargetPlan plan = est.PlanToTarget(0, 0, TARGET, -1, C_MIN, C_MAX, REL, 1e-3f, Estimator::ScoreOfStdErr);
        const std::vector<int32_t> counts = countsOf(est, plan.d_counts, npx);
        dump(prefix + ".counts.i32", counts.data(), (size_t)npx * 4);
        int64_t sum = 0;
        bool bounded = true;
        for (int32_t c : counts) sum += c, bounded = bounded && c >= C_MIN && c <= C_MAX;
        std::printf("target: total %" PRId64 " need %" PRId64 " n_open %" PRId64 " n_capped %" PRId64 " n_unjudged %" PRId64 " n_live %d n_saturated %d\n",
                    plan.target.total, plan.target.need, plan.target.n_open, plan.target.n_capped, plan.target.n_unjudged, (int)plan.target.n_live,
                    (int)plan.target.n_saturated);
        if (plan.byBudget || !bounded || sum != plan.target.total || plan.target.n_open <= 0 || plan.target.n_open >= npx ||
            plan.target.need < plan.target.total - npx * C_MIN - plan.target.n_unjudged * C_MAX) {
            std::printf("MISMATCH the plan to the target: counts sum %" PRId64 ", bounded %d, by budget %d\n", sum, (int)bounded, (int)plan.byBudget);
            return 1;
        }
        // a budget the plan fits: no fallback, the same counts
        const Estimator::TargetPlan fits = est.PlanToTarget(0, 0, TARGET, plan.target.total, C_MIN, C_MAX, REL, 1e-3f, Estimator::ScoreOfStdErr);
        if (fits.byBudget || std::memcmp(&fits.target, &plan.target, sizeof(plan.target)) != 0 || countsOf(est, fits.d_counts, npx) != counts) {
            std::printf("MISMATCH a budget equal to the plan's total changed the plan\n");
            return 1;
        }
        // ---- the budget fallback: one sample short
        const int64_t budget = plan.target.total - 1;
        const Estimator::TargetPlan fell = est.PlanToTarget(0, 0, TARGET, budget, C_MIN, C_MAX, REL, 1e-3f, Estimator::ScoreOfStdErr);
        const std::vector<int32_t> spent = countsOf(est, fell.d_counts, npx);
        sum = 0;
        for (int32_t c : spent) sum += c;
        if (!fell.byBudget || std::memcmp(&fell.target, &plan.target, sizeof(plan.target)) != 0 || fell.budgeted.status != 0 ||
            fell.budgeted.total != budget || sum != budget) {
            std::printf("MISMATCH the fallback: by budget %d, status %d, total %" PRId64 ", counts %" PRId64 ", budget %" PRId64 "\n", (int)fell.byBudget,
                        (int)fell.budgeted.status, fell.budgeted.total, sum, budget);
            return 1;
        }
        const Estimator::SamplePlan same = est.PlanSamples(0, 0, budget, C_MIN, C_MAX, REL, 1e-3f, 0);
        if (countsOf(est, same.d_counts, npx) != spent) {
            std::printf("MISMATCH the fallback's counts are not PlanSamples' for the same budget\n");
            return 1;
        }

        // ---- refusals
        try {
            est.PlanToTarget(0, 0, TARGET, -1, C_MIN, C_MAX, REL, 1e-3f, Estimator::ScoreOfDeviation);
            std::printf("MISMATCH PlanToTarget on the sample deviation was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        try {
            est.ScoreSelect(0, 0, median, REL, 1e-3f, 0, 3);
            std::printf("MISMATCH scoreOf 3 was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        try {
            est.PlanToTarget(0, 0, 0.f, -1, C_MIN, C_MAX, REL, 1e-3f, Estimator::ScoreOfStdErr);
            std::printf("MISMATCH a target of 0 was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        std::printf("plan to target ok: %dx%d, target %g\n", W, H, (double)TARGET);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
