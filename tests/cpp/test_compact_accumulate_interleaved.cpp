// The planned iteration with one struct store per sample, through the C++ host: Estimator::PlanSamples -> Estimator::CompactOffsets
// -> the "renderer" writes pixel p's sample s as ONE record {radiance, normal, albedo, padding} at slot offsets[p] + s ->
// Estimator::AccumulateCompactInterleaved.  A second Estimator takes the same samples as one compact arena per type through
// Estimator::AccumulateCompact with the same offsets.  After Upload / Denoise / Download / DownloadStatistics the "film-f" image
// and every statistics image must be the same bits in both.
//   test_compact_accumulate_interleaved [width height]     prints "compact accumulate interleaved ok" and exits 0, or names the
//                                                          first difference
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
// sample s of pixel px, channel c of stat type `type`: positive radiance, noisier towards the film's right edge and with the odd
// firefly, features in [0, 1)
float sampleOf(int type, int px, int s, int c, int width) {
    const uint32_t h = mix32((uint32_t)px * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    if (type != 0) return u;
    const float spread = 0.05f + (float)(px % width) / (float)width;
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.5f + spread * u);
}

struct Film {
    Buffer film;
    BufferRegistry reg;
    Estimator est;
    Film(int w, int h, const StatTypeConfigs &cfgs)
        : film("film", HostImage(h, w, F32C3)), reg(film),
          est(film, cfgs, 10.f, 20, /*denoiseFilm=*/true, /*acrr=*/false, /*smis=*/false, reg) {
        float *f = film.mat.ptr<float>();
        for (int i = 0; i < w * h * 3; i++) f[i] = sampleOf(0, i / 3, 1000, i % 3, w);
        est.AllocateBuffers(reg);
    }
};

bool sameBits(const HostImage &a, const HostImage &b, const std::string &what) {
    if (a.bytes() != b.bytes() || std::memcmp(a.ptr(), b.ptr(), a.bytes()) != 0) {
        std::printf("MISMATCH %s\n", what.c_str());
        return false;
    }
    return true;
}

struct DeviceArray {
    void *ptr = nullptr;
    explicit DeviceArray(size_t bytes) { check(statmc_malloc(&ptr, bytes ? bytes : 8)); }
    DeviceArray(const void *host, size_t bytes, void *stream) : DeviceArray(bytes) {
        if (bytes) check(statmc_upload(ptr, host, bytes, stream));
    }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
};

}  // namespace

int main(int argc, char **argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 61, H = argc > 2 ? std::atoi(argv[2]) : 37;
    const int npx = W * H, seed = 4;
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film compact(W, H, cfgs), records(W, H, cfgs);   // compact: interleaved records; records: one arena per type
        if (compact.est.statTypeConfigs.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", compact.est.statTypeConfigs.nEnabled);
            return 1;
        }
        for (Film *f : {&compact, &records}) f->est.EnableDeviceAccumulation((size_t)64 << 20);

        // ---- a first, uniform iteration through the records entry in both films: statistics for the plan to judge
        {
            std::vector<int32_t> pixels;
            std::vector<float> smp[3];
            for (int s = 0; s < seed; s++)
                for (int k = 0; k < npx; k++) {
                    pixels.push_back(k);
                    for (int i = 0; i < 3; i++)
                        for (int c = 0; c < 3; c++) smp[i].push_back(sampleOf(i, k, s, c, W));
                }
            for (Film *f : {&compact, &records}) {
                void *st = f->est.DeviceStream();
                DeviceArray dPixels(pixels.data(), pixels.size() * sizeof(int32_t), st);
                DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), st), d1(smp[1].data(), smp[1].size() * sizeof(float), st),
                    d2(smp[2].data(), smp[2].size() * sizeof(float), st);
                f->est.AccumulateRecords(static_cast<const int32_t *>(dPixels.ptr), (int64_t)pixels.size(),
                                         {{0, 0, static_cast<const float *>(d0.ptr)}, {1, 0, static_cast<const float *>(d1.ptr)},
                                          {2, 0, static_cast<const float *>(d2.ptr)}});
                check(statmc_synchronize(st));   // before the arrays are freed
            }
        }

        // ---- plan -> offsets -> the renderer writes one record per sample -> fold, on the compact film's stream
        void *st = compact.est.DeviceStream();
        const int64_t budget = (int64_t)npx * 5 + 3, capacity = budget + 100;   // the arenas: 100 slots nobody owns behind the total
        const Estimator::SamplePlan plan = compact.est.PlanSamples(0, 0, budget, 0, 40);
        if (plan.result.status != 0 || plan.result.total != budget) {
            std::printf("plan: status %d, total %lld of %lld\n", plan.result.status, (long long)plan.result.total, (long long)budget);
            return 1;
        }
        DeviceArray dOffsets((size_t)(npx + 1) * sizeof(int64_t));
        compact.est.CompactOffsets(plan.d_counts, INT32_MAX, static_cast<int64_t *>(dOffsets.ptr));
        std::vector<int64_t> offsets(npx + 1);
        check(statmc_download(offsets.data(), dOffsets.ptr, offsets.size() * sizeof(int64_t), st));
        check(statmc_synchronize(st));
        if (offsets[0] != 0 || offsets[npx] != budget) {
            std::printf("offsets: [0] = %lld, total %lld, budget %lld\n", (long long)offsets[0], (long long)offsets[npx], (long long)budget);
            return 1;
        }
        int longest = 0;
        struct Sample {          // what the renderer's thread stores: 40 bytes
            float radiance[3], normal[3], albedo[3];
            uint32_t padding;
        };
        static_assert(sizeof(Sample) == 40, "three RGB fields and a padding word");
        Sample unowned;
        std::memset(&unowned, 0xFF, sizeof(unowned));   // NaN everywhere: slots nobody owns
        std::vector<Sample> queue((size_t)capacity, unowned);
        std::vector<float> smp[3];
        for (auto &a : smp) a.assign((size_t)capacity * 3, -1.f);
        for (int k = 0; k < npx; k++) {
            const int c = (int)(offsets[k + 1] - offsets[k]);
            if (c < 0 || c > 40) {
                std::printf("offsets: pixel %d has %d samples\n", k, c);
                return 1;
            }
            longest = c > longest ? c : longest;
            for (int s = 0; s < c; s++) {
                Sample &r = queue[(size_t)(offsets[k] + s)];
                for (int ch = 0; ch < 3; ch++) {
                    r.radiance[ch] = smp[0][(size_t)(offsets[k] + s) * 3 + ch] = sampleOf(0, k, seed + s, ch, W);
                    r.normal[ch] = smp[1][(size_t)(offsets[k] + s) * 3 + ch] = sampleOf(1, k, seed + s, ch, W);
                    r.albedo[ch] = smp[2][(size_t)(offsets[k] + s) * 3 + ch] = sampleOf(2, k, seed + s, ch, W);
                }
            }
        }
        {
            DeviceArray dQueue(queue.data(), queue.size() * sizeof(Sample), st);
            compact.est.AccumulateCompactInterleaved(capacity, dQueue.ptr, Estimator::RecordLayout{(int)sizeof(Sample), /* pixelOffset: ignored */ -1},
                                                     {{0, 0, (int)offsetof(Sample, radiance)}, {1, 0, (int)offsetof(Sample, normal)},
                                                      {2, 0, (int)offsetof(Sample, albedo)}},
                                                     static_cast<const int64_t *>(dOffsets.ptr), 16);
            check(statmc_synchronize(st));
            void *rst = records.est.DeviceStream();
            DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), rst), d1(smp[1].data(), smp[1].size() * sizeof(float), rst),
                d2(smp[2].data(), smp[2].size() * sizeof(float), rst);
            records.est.AccumulateCompact(capacity, {{0, 0, d0.ptr, STATMC_SAMPLES_F32}, {1, 0, d1.ptr, STATMC_SAMPLES_F32}, {2, 0, d2.ptr, STATMC_SAMPLES_F32}},
                                          static_cast<const int64_t *>(dOffsets.ptr), 16);
            check(statmc_synchronize(rst));
        }
        for (Film *f : {&compact, &records}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        bool ok = true;
        const Estimator &a = compact.est, &o = records.est;
        ok &= sameBits(a.filmFilteredBuffer.mat, o.filmFilteredBuffer.mat, "film-f");
        for (unsigned char i = 0; i < a.statTypeConfigs.nEnabled; i++) {
            const std::string pre = "t" + std::to_string(i) + "-b0";
            ok &= sameBits(a.nBuffers[i][0].mat, o.nBuffers[i][0].mat, pre + "-n");
            ok &= sameBits(a.meanBuffers[i][0].mat, o.meanBuffers[i][0].mat, pre + "-mean");
            ok &= sameBits(a.m2Buffers[i][0].mat, o.m2Buffers[i][0].mat, pre + "-m2");
            ok &= sameBits(a.m3Buffers[i][0].mat, o.m3Buffers[i][0].mat, pre + "-m3");
            ok &= sameBits(a.filmBuffers[i][0].mat, o.filmBuffers[i][0].mat, pre + "-film-mean");
            ok &= sameBits(a.filmM2Buffers[i][0].mat, o.filmM2Buffers[i][0].mat, pre + "-film-m2");
        }
        const int32_t *n = a.nBuffers[0][0].mat.ptr<int32_t>();
        for (int k = 0; k < npx && ok; k++)
            if (n[k] != seed + (int)(offsets[k + 1] - offsets[k])) {
                std::printf("MISMATCH count %d at pixel %d, fed %d\n", n[k], k, seed + (int)(offsets[k + 1] - offsets[k]));
                ok = false;
            }
        if (!ok) return 1;
        std::printf("compact accumulate interleaved ok: %dx%d, %lld samples by the plan, longest run %d\n", W, H, (long long)budget, longest);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
