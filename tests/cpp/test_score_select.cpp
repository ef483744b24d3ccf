// Estimator::ScoreSelect / Estimator::ScoreCountAbove from the C++ host: a stopping rule's order statistics of the radiance score.
// A first batch of 6 samples per pixel; a select of five ranks of the relative score and the counts above three thresholds, one of
// them the selected median.  Checked here: n_below <= rank < n_below + n_equal, value_bits non-decreasing in rank, the count above
// the median equal to n_px - n_below - n_equal, the class counts equal to PlanSamples', and the score image computed once for
// PlanSamples + ScoreSelect + ScoreCountAbove of the same type and metric, and again behind every way the statistics change: an
// accumulation, another metric, a flush of staged samples, ResetStatistics, CombineStatistics, CombineRecords, a second
// EnableDeviceAccumulation, PoolStatistics into the film -- and on every call once a descriptor was handed out through
// DeviceStatistics: a C-ABI statmc_accumulate through a descriptor obtained earlier is seen by the next PlanSamples and ScoreSelect.
// Dumped for tests/test_score_select_gpu.py, which scores the same statistics through the Python entry and compares with the numpy
// restatement:
//   <prefix>.n.i32  <prefix>.film_mean.f32  <prefix>.film_m2.f32   the radiance statistics the scores were made from
//   test_score_select width height prefix    prints "classes: ...", one "select: ..." line per rank, one "above: ..." line per
//                                            threshold and "score select ok", exits 0; or names the difference
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
// sample s of pixel (x, y), channel c of stat type `type`: radiance whose spread grows across the film
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

statmc_select_result fetch(Estimator &est, const statmc_select_result *d) {
    statmc_select_result r;
    check(statmc_download(&r, d, sizeof(r), est.DeviceStream()));
    est.Synchronize();
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::printf("usage: %s width height prefix\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), FIRST = 6;
    const std::string prefix = argv[3];
    const int64_t npx = (int64_t)W * H;
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        Film f(W, H, makeStatTypeConfigs(p));
        Estimator &est = f.est;
        try {   // the statistics must live on the device first
            est.ScoreSelect(0, 0, {0});
            std::printf("ScoreSelect before EnableDeviceAccumulation did not throw\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        est.EnableDeviceAccumulation((size_t)64 << 20);
        accumulate(est, W, H, 0, FIRST);
        est.DownloadStatistics();
        est.Synchronize();
        dump(prefix + ".n.i32", est.nBuffers[0][0].mat.ptr(), (size_t)npx * 4);
        dump(prefix + ".film_mean.f32", est.filmBuffers[0][0].mat.ptr(), (size_t)npx * 12);
        dump(prefix + ".film_m2.f32", est.filmM2Buffers[0][0].mat.ptr(), (size_t)npx * 12);

        // one score image serves the plan, the select and the counts
        const size_t images0 = est.ScoreImagesComputed();
        const Estimator::SamplePlan plan = est.PlanSamples(0, 0, npx * 4, 1, 8);
        const std::vector<int64_t> ranks = {npx / 2, 0, npx - 1, Estimator::NearestRank(0.95, npx), npx / 2};
        const statmc_select_result r = fetch(est, est.ScoreSelect(0, 0, ranks));
        float median;
        std::memcpy(&median, &r.value_bits[0], sizeof(median));
        const std::vector<float> thresholds = {0.f, median, HUGE_VALF};
        int64_t above[3];
        check(statmc_download(above, est.ScoreCountAbove(0, 0, thresholds), sizeof(above), est.DeviceStream()));
        est.Synchronize();
        if (est.ScoreImagesComputed() != images0 + 1) {
            std::printf("MISMATCH %zu score images computed for one plan, one select and one count of the same statistics\n",
                        est.ScoreImagesComputed() - images0);
            return 1;
        }
        std::printf("classes: px %" PRId64 " live %" PRId64 " saturated %" PRId64 "\n", r.n_px, r.n_live, r.n_saturated);
        if (r.n_px != npx || r.n_ranks != (int)ranks.size() || r.n_live != plan.result.n_live || r.n_saturated != plan.result.n_saturated) {
            std::printf("MISMATCH n_px %" PRId64 ", n_ranks %d, or the classes differ from the plan's %d / %d\n", r.n_px, (int)r.n_ranks,
                        (int)plan.result.n_live, (int)plan.result.n_saturated);
            return 1;
        }
        for (int i = 0; i < STATMC_SELECT_MAX_RANKS; i++) {
            if (i >= r.n_ranks) {
                if (r.rank[i] || r.value_bits[i] || r.n_below[i] || r.n_equal[i]) {
                    std::printf("MISMATCH slot %d behind the ranks is not zero\n", i);
                    return 1;
                }
                continue;
            }
            std::printf("select: rank %" PRId64 " value 0x%08x below %" PRId64 " equal %" PRId64 "\n", r.rank[i], (unsigned)r.value_bits[i], r.n_below[i],
                        r.n_equal[i]);
            if (r.rank[i] != ranks[(size_t)i] || !(r.n_below[i] <= r.rank[i] && r.rank[i] < r.n_below[i] + r.n_equal[i])) {
                std::printf("MISMATCH rank %d: n_below <= rank < n_below + n_equal does not hold\n", i);
                return 1;
            }
            for (int j = 0; j < r.n_ranks; j++)
                if (r.rank[j] <= r.rank[i] && r.value_bits[j] > r.value_bits[i]) {
                    std::printf("MISMATCH value_bits is not monotone in rank (%d, %d)\n", j, i);
                    return 1;
                }
        }
        for (int i = 0; i < 3; i++) {
            uint32_t b;
            std::memcpy(&b, &thresholds[(size_t)i], sizeof(b));
            std::printf("above: threshold 0x%08x count %" PRId64 "\n", (unsigned)b, above[i]);
        }
        if (above[1] != npx - r.n_below[0] - r.n_equal[0] || above[2] != 0 || above[0] < above[1]) {
            std::printf("MISMATCH the counts above the median / +inf / 0 do not fit the select\n");
            return 1;
        }
        // the same select again: the same bits, in the same member struct, still the one score image
        const statmc_select_result *d_first = est.ScoreSelect(0, 0, ranks);
        const statmc_select_result again = fetch(est, d_first);
        if (std::memcmp(&again, &r, sizeof(r)) != 0 || est.ScoreImagesComputed() != images0 + 1) {
            std::printf("MISMATCH the second select differs from the first, or scored again\n");
            return 1;
        }
        // another metric is another image; more samples make the image stale: scored again both times, and the values move
        const statmc_select_result absolute = fetch(est, est.ScoreSelect(0, 0, ranks, STATMC_SCORE_ABSOLUTE));
        if (est.ScoreImagesComputed() != images0 + 2 || absolute.value_bits[0] == r.value_bits[0]) {
            std::printf("MISMATCH the absolute metric reused the relative score image\n");
            return 1;
        }
        accumulate(est, W, H, FIRST, 10);
        const statmc_select_result later = fetch(est, est.ScoreSelect(0, 0, ranks, STATMC_SCORE_ABSOLUTE));
        if (est.ScoreImagesComputed() != images0 + 3 || later.value_bits[0] == absolute.value_bits[0]) {
            std::printf("MISMATCH the select behind an accumulation reused a stale score image\n");
            return 1;
        }
        // ---- every other way this Estimator's statistics change makes the image stale: a select of the same arguments scores
        // again and its median moves.  (Type 0's descriptor was never handed out by est: the reuse is on.)
        uint32_t last = later.value_bits[0];
        size_t images = est.ScoreImagesComputed();
        bool fine = true;
        auto stale = [&](Estimator &e, const char *what, uint32_t &lastValue, size_t &count) {
            const statmc_select_result now = fetch(e, e.ScoreSelect(0, 0, {(int64_t)e.width * e.height / 2}, STATMC_SCORE_ABSOLUTE));
            if (e.ScoreImagesComputed() != count + 1 || now.value_bits[0] == lastValue) {
                std::printf("MISMATCH the select behind %s reused a stale score image (median 0x%08x -> 0x%08x, %zu scored)\n", what, (unsigned)lastValue,
                            (unsigned)now.value_bits[0], e.ScoreImagesComputed() - count);
                fine = false;
            }
            const statmc_select_result same = fetch(e, e.ScoreSelect(0, 0, {(int64_t)e.width * e.height / 2}, STATMC_SCORE_ABSOLUTE));
            if (e.ScoreImagesComputed() != count + 1 || same.value_bits[0] != now.value_bits[0]) {
                std::printf("MISMATCH the second select behind %s scored again or differs\n", what);
                fine = false;
            }
            lastValue = now.value_bits[0];
            count = e.ScoreImagesComputed();
        };
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        {   // a flush of staged samples: three more samples on every pixel of the radiance type through tiles, merged, not flushed yet
            for (int ty = 0; ty < H; ty += 16)
                for (int tx = 0; tx < W; tx += 16) {
                    std::vector<StatTile<Vec3>> tiles =
                        est.GetTiles<Vec3>(Bounds2i(Point2i(tx, ty), Point2i(std::min(tx + 16, W), std::min(ty + 16, H))), cfgs[Radiance].bounceEnd);
                    for (int y = ty; y < std::min(ty + 16, H); y++)
                        for (int x = tx; x < std::min(tx + 16, W); x++)
                            for (int s = 0; s < 3; s++)
                                tiles[0].AddTransformSampleM3(Point2i(x, y), Vec3{sampleOf(0, x, y, 100 + s, 0, W), sampleOf(0, x, y, 100 + s, 1, W),
                                                                                 sampleOf(0, x, y, 100 + s, 2, W)});
                    est.MergeTransformTiles(tiles, cfgs[Radiance]);
                }
            stale(est, "a flush of staged samples", last, images);
        }
        Film g(W, H, cfgs);   // a second film of the same size, its descriptors handed out before anything is scored
        g.est.EnableDeviceAccumulation((size_t)64 << 20);
        statmc_stat_type kept[3] = {g.est.DeviceStatistics(0, 0), g.est.DeviceStatistics(1, 0), g.est.DeviceStatistics(2, 0)};
        auto accumulateKept = [&](int s0, int S) {   // the C-ABI entry through descriptors obtained earlier: g.est sees nothing of it
            std::vector<float> arena[3];
            for (int i = 0; i < 3; i++)
                for (int s = s0; s < s0 + S; s++)
                    for (int k = 0; k < W * H; k++)
                        for (int c = 0; c < 3; c++) arena[i].push_back(sampleOf(i, k % W, k / W, s, c, W));
            void *st = g.est.DeviceStream();
            DeviceArray d0(arena[0].data(), arena[0].size() * sizeof(float), st), d1(arena[1].data(), arena[1].size() * sizeof(float), st),
                d2(arena[2].data(), arena[2].size() * sizeof(float), st);
            const void *ptrs[3] = {d0.ptr, d1.ptr, d2.ptr};
            for (int i = 0; i < 3; i++) kept[i].samples = static_cast<const float *>(ptrs[i]), kept[i].n_samples = S;
            check(statmc_accumulate((uint16_t)W, (uint16_t)H, kept, 3, st));
            check(statmc_synchronize(st));
        };
        {
            accumulateKept(0, 4);
            const Estimator::SamplePlan p1 = g.est.PlanSamples(0, 0, npx * 4, 1, 8);
            const statmc_select_result s1 = fetch(g.est, g.est.ScoreSelect(0, 0, {npx / 2}));
            std::vector<int32_t> c1((size_t)npx), c2((size_t)npx);
            check(statmc_download(c1.data(), p1.d_counts, (size_t)npx * 4, g.est.DeviceStream()));
            g.est.Synchronize();
            accumulateKept(4, 12);
            const statmc_select_result s2 = fetch(g.est, g.est.ScoreSelect(0, 0, {npx / 2}));   // the select first: no plan has scored since
            const Estimator::SamplePlan p2 = g.est.PlanSamples(0, 0, npx * 4, 1, 8);
            check(statmc_download(c2.data(), p2.d_counts, (size_t)npx * 4, g.est.DeviceStream()));
            g.est.Synchronize();
            // what a fresh look at the statistics gives: a third film's own entries on the same 16 samples
            Film h(W, H, cfgs);
            h.est.EnableDeviceAccumulation((size_t)64 << 20);
            accumulate(h.est, W, H, 0, 4);
            accumulate(h.est, W, H, 4, 12);
            const statmc_select_result want = fetch(h.est, h.est.ScoreSelect(0, 0, {npx / 2}));
            if (s2.value_bits[0] == s1.value_bits[0] || s2.value_bits[0] != want.value_bits[0] || c1 == c2) {
                std::printf("MISMATCH a select or plan behind a C-ABI accumulation through a kept descriptor saw the old statistics\n");
                fine = false;
            }
        }
        {   // ResetStatistics, then the statistics of g combined into the empty film; CombineRecords; a second EnableDeviceAccumulation
            est.ResetStatistics(0);
            stale(est, "ResetStatistics", last, images);
            est.ResetStatistics(1), est.ResetStatistics(2);
            est.CombineStatistics(g.est);
            stale(est, "CombineStatistics", last, images);
            const int32_t nrec = (int32_t)npx;
            std::vector<int32_t> pixels((size_t)nrec);
            for (int32_t k = 0; k < nrec; k++) pixels[(size_t)k] = k;
            DeviceArray d_pixels(pixels.data(), pixels.size() * 4, est.DeviceStream());
            const size_t dwords = statmc_state_dwords(cfgs[Radiance].nChannels, cfgs[Radiance].maxMoment, cfgs[Radiance].transform);
            std::vector<int32_t> zeros((size_t)nrec * dwords, 0);
            DeviceArray d_states(zeros.data(), zeros.size() * 4, est.DeviceStream());
            g.est.GatherStates(static_cast<const int32_t *>(d_pixels.ptr), nrec, {{0, 0, d_states.ptr}});
            g.est.Synchronize();
            est.CombineRecords(static_cast<const int32_t *>(d_pixels.ptr), nrec, {{0, 0, d_states.ptr}});
            stale(est, "CombineRecords", last, images);
            est.Synchronize();
            est.EnableDeviceAccumulation((size_t)64 << 20);
            stale(est, "a second EnableDeviceAccumulation", last, images);
        }
        {   // PoolStatistics writes the coarse film
            Film c((W + 1) / 2, (H + 1) / 2, cfgs);
            c.est.EnableDeviceAccumulation((size_t)64 << 20);
            const statmc_select_result empty = fetch(c.est, c.est.ScoreSelect(0, 0, {0}, STATMC_SCORE_ABSOLUTE));
            uint32_t coarseLast = empty.value_bits[0];
            size_t coarseImages = c.est.ScoreImagesComputed();
            g.est.PoolStatistics(c.est, 2);
            stale(c.est, "PoolStatistics into it", coarseLast, coarseImages);
        }
        if (!fine) return 1;
        std::printf("score select ok: %dx%d, %d first\n", W, H, FIRST);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
