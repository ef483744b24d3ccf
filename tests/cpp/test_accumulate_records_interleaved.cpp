// An Estimator fed through Estimator::AccumulateRecordsInterleaved -- a wavefront renderer's queue as it holds it, one struct per
// finished sample -- against one fed through Estimator::AccumulateRecords with the same samples de-interleaved into one array per
// stat type (half fields widened to fp32 on the host): after Upload / Denoise / Download / DownloadStatistics the "film-f" image and
// every statistics image must be the same bits.  Two batches, so the second starts from n > 0; an odd film size; the records visit
// the pixels in a scrambled order that differs from sample to sample, with skipped records in between; the radiance type is folded
// with its pre-pass epilogue.  The record: 36 bytes, the normal first (fp32), the pixel index in the middle, the radiance (fp32)
// behind it, two bytes of padding, the albedo in half at an offset that is a multiple of 2 but not of 4.
//   test_accumulate_records_interleaved [width height]     prints "accumulate records interleaved ok" and exits 0, or names the
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
uint32_t hashOf(int type, int px, int s, int c) { return mix32((uint32_t)px * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu)); }
// radiance and normal: fp32
float sampleOf(int type, int px, int s, int c) {
    const uint32_t h = hashOf(type, px, s, c);
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    if (type != 0) return u;
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.01f + u * u);
}
// albedo: the bits of a non-negative half below 1 -- exponents 0 .. 14, subnormals and zero included
uint16_t halfBitsOf(int px, int s, int c) { return (uint16_t)(hashOf(2, px, s, c) % 0x3c00u); }
// every finite half is an fp32 value
float widen(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const float mag = e == 0 ? (float)m * (1.f / 16777216.f) : (float)(1024 + m) * (1.f / 1024.f) * (e >= 15 ? (float)(1 << (e - 15)) : 1.f / (float)(1 << (15 - e)));
    return (h & 0x8000) ? -mag : mag;
}

#pragma pack(push, 1)
struct QueueEntry {
    float normal[3];
    int32_t pixel;
    float radiance[3];
    uint16_t pad0;
    uint16_t albedo[3];
};
#pragma pack(pop)
static_assert(sizeof(QueueEntry) == 36 && offsetof(QueueEntry, albedo) == 30, "the record this test describes");

struct Film {
    Buffer film;
    BufferRegistry reg;
    Estimator est;
    Film(int w, int h, const StatTypeConfigs &cfgs)
        : film("film", HostImage(h, w, F32C3)), reg(film),
          est(film, cfgs, 10.f, 20, /*denoiseFilm=*/true, /*acrr=*/false, /*smis=*/false, reg) {
        float *f = film.mat.ptr<float>();
        for (int i = 0; i < w * h * 3; i++) f[i] = sampleOf(0, i / 3, 1000, i % 3);
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
    DeviceArray(const void *host, size_t bytes, void *stream) {
        check(statmc_malloc(&ptr, bytes));
        check(statmc_upload(ptr, host, bytes, stream));
    }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
};

}  // namespace

int main(int argc, char **argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 61, H = argc > 2 ? std::atoi(argv[2]) : 37;
    const int batches[2] = {5, 7};
    const int npx = W * H;
    if (npx % 7919 == 0) {   // the records visit the pixels in the order k -> (7919 k + ...) mod npx: a permutation otherwise
        std::printf("film size not supported by this test's pixel permutation\n");
        return 1;
    }
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film arrays(W, H, cfgs), queue(W, H, cfgs);
        const auto &kept = arrays.est.statTypeConfigs;
        if (kept.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", kept.nEnabled);
            return 1;
        }
        const Estimator::RecordLayout layout{(int)sizeof(QueueEntry), (int)offsetof(QueueEntry, pixel)};
        const std::vector<Estimator::RecordField> fields = {{0, 0, (int)offsetof(QueueEntry, radiance), STATMC_SAMPLES_F32, true},
                                                            {1, 0, (int)offsetof(QueueEntry, normal), STATMC_SAMPLES_F32},
                                                            {2, 0, (int)offsetof(QueueEntry, albedo), STATMC_SAMPLES_F16}};
        try {   // the statistics must live on the device first
            queue.est.AccumulateRecordsInterleaved(nullptr, 0, layout, fields);
            std::printf("AccumulateRecordsInterleaved before EnableDeviceAccumulation did not throw\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        arrays.est.EnableDeviceAccumulation((size_t)64 << 20);
        queue.est.EnableDeviceAccumulation((size_t)64 << 20);
        try {   // a layout the library refuses comes back as its error
            Estimator::RecordLayout bad = layout;
            bad.stride = 34;
            queue.est.AccumulateRecordsInterleaved(nullptr, 0, bad, fields);
            std::printf("a stride of 34 was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID || std::strstr(e.what(), "stride") == nullptr) throw;
        }

        int s0 = 0;
        for (const int S : batches) {
            // the queue of finished samples: sample s of every pixel, the pixels in an order that depends on s (ascending record
            // index inside a pixel is ascending s), every seventh record a skipped one
            std::vector<QueueEntry> entries;
            std::vector<int32_t> pixels;
            std::vector<float> smp[3];
            for (int s = s0; s < s0 + S; s++)
                for (int k = 0; k < npx; k++) {
                    if (entries.size() % 7 == 3) {
                        QueueEntry dead;
                        std::memset(&dead, 0x7f, sizeof(dead));      // never folded
                        dead.pixel = entries.size() % 2 ? -1 : npx + 7;
                        entries.push_back(dead);
                        pixels.push_back(dead.pixel);
                        for (auto &v : smp) v.insert(v.end(), {1e30f, -1.f, 7.f});
                    }
                    const int px = (int)(((int64_t)k * 7919 + (int64_t)s * 104729) % npx);
                    QueueEntry e;
                    std::memset(&e, 0xee, sizeof(e));
                    e.pixel = px;
                    for (int c = 0; c < 3; c++) {
                        e.radiance[c] = sampleOf(0, px, s, c);
                        e.normal[c] = sampleOf(1, px, s, c);
                        e.albedo[c] = halfBitsOf(px, s, c);
                        smp[0].push_back(e.radiance[c]);
                        smp[1].push_back(e.normal[c]);
                        smp[2].push_back(widen(e.albedo[c]));
                    }
                    entries.push_back(e);
                    pixels.push_back(px);
                }
            {
                void *st = arrays.est.DeviceStream();
                DeviceArray dPixels(pixels.data(), pixels.size() * sizeof(int32_t), st);
                DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), st), d1(smp[1].data(), smp[1].size() * sizeof(float), st),
                    d2(smp[2].data(), smp[2].size() * sizeof(float), st);
                arrays.est.AccumulateRecords(static_cast<const int32_t *>(dPixels.ptr), (int64_t)pixels.size(),
                                             {{0, 0, static_cast<const float *>(d0.ptr), true},
                                              {1, 0, static_cast<const float *>(d1.ptr)},
                                              {2, 0, static_cast<const float *>(d2.ptr)}});
                check(statmc_synchronize(st));   // before the arrays are freed
            }
            {
                void *st = queue.est.DeviceStream();
                DeviceArray dEntries(entries.data(), entries.size() * sizeof(QueueEntry), st);
                queue.est.AccumulateRecordsInterleaved(dEntries.ptr, (int64_t)entries.size(), layout, fields);
                check(statmc_synchronize(st));
            }
            s0 += S;
        }
        for (Film *f : {&arrays, &queue}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        bool ok = sameBits(arrays.est.filmFilteredBuffer.mat, queue.est.filmFilteredBuffer.mat, "film-f");
        const Estimator &a = arrays.est, &b = queue.est;
        for (unsigned char i = 0; i < kept.nEnabled; i++) {
            const std::string pre = "t" + std::to_string(i) + "-b0";
            ok &= sameBits(a.nBuffers[i][0].mat, b.nBuffers[i][0].mat, pre + "-n");
            ok &= sameBits(a.meanBuffers[i][0].mat, b.meanBuffers[i][0].mat, pre + "-mean");
            ok &= sameBits(a.m2Buffers[i][0].mat, b.m2Buffers[i][0].mat, pre + "-m2");
            ok &= sameBits(a.m3Buffers[i][0].mat, b.m3Buffers[i][0].mat, pre + "-m3");
            ok &= sameBits(a.filmBuffers[i][0].mat, b.filmBuffers[i][0].mat, pre + "-film-mean");
            ok &= sameBits(a.filmM2Buffers[i][0].mat, b.filmM2Buffers[i][0].mat, pre + "-film-m2");
        }
        // the counts are what was fed, and the albedo's mean is not all zero (the half field was read where it lies)
        const int32_t *n = b.nBuffers[0][0].mat.ptr<int32_t>();
        for (int k = 0; k < npx; k++)
            if (n[k] != batches[0] + batches[1]) {
                std::printf("MISMATCH count %d at pixel %d\n", n[k], k);
                ok = false;
                break;
            }
        const float *albedo = b.meanBuffers[2][0].mat.ptr<float>();
        double sum = 0;
        for (int k = 0; k < npx * 3; k++) sum += albedo[k];
        if (!(sum > 0.01 * npx && sum < 3.0 * npx)) {
            std::printf("MISMATCH albedo mean sums to %g\n", sum);
            ok = false;
        }
        if (!ok) return 1;
        std::printf("accumulate records interleaved ok: %dx%d, %d + %d samples, %d types\n", W, H, batches[0], batches[1], kept.nEnabled);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
