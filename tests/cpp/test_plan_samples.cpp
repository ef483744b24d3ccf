// Estimator::PlanSamples followed by Estimator::AccumulateFilm(S, buffers, d_counts): the loop statistics -> counts -> counted
// accumulation from the C++ host.  A first batch of 6 samples per pixel; a plan of width * height * capacity / 2 further samples with
// 1 .. capacity per pixel from the radiance statistics; a capacity-deep arena accumulated with the planned count image.  Checked here:
// status 0, the counts sum to the budget and keep their bounds, and every type's n grows by exactly the planned count at every pixel.
// Dumped for tests/test_plan_gpu.py, which plans the same statistics through the Python entry and compares the bits:
//   <prefix>.n.i32  <prefix>.film_mean.f32  <prefix>.film_m2.f32   the radiance statistics the plan was made from
//   <prefix>.counts.i32                                           the planned count image
//   test_plan_samples width height capacity prefix     prints "result: ..." and "plan samples ok", exits 0; or names the difference
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
// sample s of pixel (x, y), channel c of stat type `type`: radiance whose spread grows across the film, so the plan is uneven
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
void accumulate(Estimator &est, int W, int H, int s0, int S, const int32_t *d_counts) {
    std::vector<float> arena[3];
    for (int i = 0; i < 3; i++)
        for (int s = s0; s < s0 + S; s++)
            for (int k = 0; k < W * H; k++)
                for (int c = 0; c < 3; c++) arena[i].push_back(sampleOf(i, k % W, k / W, s, c, W));
    void *st = est.DeviceStream();
    DeviceArray d0(arena[0].data(), arena[0].size() * sizeof(float), st), d1(arena[1].data(), arena[1].size() * sizeof(float), st),
        d2(arena[2].data(), arena[2].size() * sizeof(float), st);
    est.AccumulateFilm(S, {{0, 0, d0.ptr, STATMC_SAMPLES_F32}, {1, 0, d1.ptr, STATMC_SAMPLES_F32}, {2, 0, d2.ptr, STATMC_SAMPLES_F32}}, d_counts);
    check(statmc_synchronize(st));   // before the arrays are freed
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) {
        std::printf("usage: %s width height capacity prefix\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), CAP = std::atoi(argv[3]), FIRST = 6;
    const std::string prefix = argv[4];
    const size_t npx = (size_t)W * H;
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        Film f(W, H, makeStatTypeConfigs(p));
        Estimator &est = f.est;
        try {   // the statistics must live on the device first
            est.PlanSamples(0, 0, 1, 0, 1);
            std::printf("PlanSamples before EnableDeviceAccumulation did not throw\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        est.EnableDeviceAccumulation((size_t)64 << 20);
        accumulate(est, W, H, 0, FIRST, nullptr);
        est.DownloadStatistics();
        est.Synchronize();
        std::vector<int32_t> before[3];
        for (int i = 0; i < 3; i++) before[i].assign(est.nBuffers[i][0].mat.ptr<int32_t>(), est.nBuffers[i][0].mat.ptr<int32_t>() + npx);
        dump(prefix + ".n.i32", est.nBuffers[0][0].mat.ptr(), npx * 4);
        dump(prefix + ".film_mean.f32", est.filmBuffers[0][0].mat.ptr(), npx * 12);
        dump(prefix + ".film_m2.f32", est.filmM2Buffers[0][0].mat.ptr(), npx * 12);

        const int64_t budget = (int64_t)npx * (CAP / 2);
        const Estimator::SamplePlan plan = est.PlanSamples(0, 0, budget, 1, CAP);
        const statmc_plan_result &r = plan.result;
        std::printf("result: total %" PRId64 " budget %" PRId64 " level 0x%08x status %d live %d saturated %d\n", r.total, r.budget,
                    (unsigned)r.level_bits, (int)r.status, (int)r.n_live, (int)r.n_saturated);
        std::vector<int32_t> counts(npx);
        check(statmc_download(counts.data(), plan.d_counts, npx * 4, est.DeviceStream()));
        est.Synchronize();
        dump(prefix + ".counts.i32", counts.data(), npx * 4);
        int64_t sum = 0;
        for (int32_t c : counts) {
            if (c < 1 || c > CAP) {
                std::printf("MISMATCH a count of %d outside 1 .. %d\n", c, CAP);
                return 1;
            }
            sum += c;
        }
        if (r.status != 0 || r.total != budget || r.budget != budget || sum != budget) {
            std::printf("MISMATCH status %d, total %" PRId64 ", sum %" PRId64 ", budget %" PRId64 "\n", (int)r.status, r.total, sum, budget);
            return 1;
        }
        // the same plan again: the same bits, in the same member image
        const Estimator::SamplePlan again = est.PlanSamples(0, 0, budget, 1, CAP);
        std::vector<int32_t> counts2(npx);
        check(statmc_download(counts2.data(), again.d_counts, npx * 4, est.DeviceStream()));
        est.Synchronize();
        if (again.d_counts != plan.d_counts || counts2 != counts || std::memcmp(&again.result, &plan.result, sizeof(plan.result)) != 0) {
            std::printf("MISMATCH the second plan differs from the first\n");
            return 1;
        }

        accumulate(est, W, H, FIRST, CAP, plan.d_counts);
        est.DownloadStatistics();
        est.Synchronize();
        for (int i = 0; i < 3; i++) {
            const int32_t *n = est.nBuffers[i][0].mat.ptr<int32_t>();
            for (size_t k = 0; k < npx; k++)
                if (n[k] - before[i][k] != counts[k]) {
                    std::printf("MISMATCH type %d pixel %zu: n grew by %d, planned %d\n", i, k, n[k] - before[i][k], counts[k]);
                    return 1;
                }
        }
        std::printf("plan samples ok: %dx%d, %d first, capacity %d\n", W, H, FIRST, CAP);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
