// Estimator::AccumulateRecords(..., splitAbove) and Estimator::AccumulateRecordsInterleaved(..., splitAbove) against the C entries
// they stand for: four Estimators get the same queue -- two batches, so the second starts from n > 0; every pixel a few samples and
// a handful of pixels (the first, the last, the two sides of a wave's edge) a few hundred, in a scrambled order with skipped
// records in between; the radiance type with its pre-pass epilogue --
//   1  through AccumulateRecords(d_pixels, n, buffers, splitAbove)
//   2  through statmc_accumulate_records_split on the descriptors of DeviceStatistics
//   3  through AccumulateRecordsInterleaved(d_records, n, layout, fields, splitAbove)
//   4  through statmc_accumulate_records_interleaved_split on the same descriptors
// and after Upload / Denoise / Download / DownloadStatistics every statistics image and "film-f" must be the same bits in all
// four.  A fifth, fed through the sequential AccumulateRecords, must hold the same counts and -- the long pixels were split --
// not the same bits.  splitAbove = 0 must come back as STATMC_ERR_INVALID naming split_above.
//   test_accumulate_records_split [width height]     prints "accumulate records split ok" and exits 0, or names the first difference
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
float sampleOf(int type, int px, int s, int c) {
    const uint32_t h = mix32((uint32_t)px * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    if (type != 0) return u;
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.01f + u * u);
}

struct QueueEntry {
    float normal[3];
    int32_t pixel;
    float radiance[3];
    float albedo[3];
};
static_assert(sizeof(QueueEntry) == 40, "the record this test describes");

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
        est.EnableDeviceAccumulation((size_t)64 << 20);
    }
};

bool sameBits(const HostImage &a, const HostImage &b) { return a.bytes() == b.bytes() && std::memcmp(a.ptr(), b.ptr(), a.bytes()) == 0; }

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
    const int npx = W * H, kSplitAbove = 16, kShort = 3, kLong = 333;
    if (npx % 7919 == 0 || npx < 130) {
        std::printf("film size not supported by this test\n");
        return 1;
    }
    const int longPixels[] = {0, 63, 64, 65, npx - 1};
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film viaArrays(W, H, cfgs), viaC(W, H, cfgs), viaQueue(W, H, cfgs), viaQueueC(W, H, cfgs), sequential(W, H, cfgs);
        if (viaArrays.est.statTypeConfigs.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", viaArrays.est.statTypeConfigs.nEnabled);
            return 1;
        }
        const Estimator::RecordLayout layout{(int)sizeof(QueueEntry), (int)offsetof(QueueEntry, pixel)};
        const std::vector<Estimator::RecordField> fields = {{0, 0, (int)offsetof(QueueEntry, radiance), STATMC_SAMPLES_F32, true},
                                                            {1, 0, (int)offsetof(QueueEntry, normal), STATMC_SAMPLES_F32},
                                                            {2, 0, (int)offsetof(QueueEntry, albedo), STATMC_SAMPLES_F32}};
        for (int which = 0; which < 2; which++) {
            try {
                if (which == 0) viaArrays.est.AccumulateRecords(nullptr, 0, {}, 0);
                else viaQueue.est.AccumulateRecordsInterleaved(nullptr, 0, layout, fields, 0);
                std::printf("splitAbove = 0 was not refused (%d)\n", which);
                return 1;
            } catch (const Error &e) {
                if (e.code != STATMC_ERR_INVALID || std::strstr(e.what(), "split_above") == nullptr) throw;
            }
        }

        std::vector<int> fed(npx, 0);
        for (int batch = 0; batch < 2; batch++) {
            // sample s of every pixel for s < kShort, of the long pixels for s < kLong; the pixels in an order that depends on s
            std::vector<QueueEntry> entries;
            std::vector<int32_t> pixels;
            std::vector<float> smp[3];
            auto push = [&](int px, int s) {
                if (entries.size() % 7 == 3) {
                    QueueEntry dead;
                    std::memset(&dead, 0x7f, sizeof(dead));      // never folded
                    dead.pixel = entries.size() % 2 ? -1 : npx + 7;
                    entries.push_back(dead);
                    pixels.push_back(dead.pixel);
                    for (auto &v : smp) v.insert(v.end(), {1e30f, -1.f, 7.f});
                }
                QueueEntry e;
                e.pixel = px;
                for (int c = 0; c < 3; c++) {
                    e.radiance[c] = sampleOf(0, px, s + 1000 * batch, c);
                    e.normal[c] = sampleOf(1, px, s + 1000 * batch, c);
                    e.albedo[c] = sampleOf(2, px, s + 1000 * batch, c);
                    smp[0].push_back(e.radiance[c]);
                    smp[1].push_back(e.normal[c]);
                    smp[2].push_back(e.albedo[c]);
                }
                entries.push_back(e);
                pixels.push_back(px);
                fed[px]++;
            };
            for (int s = 0; s < kLong; s++) {
                if (s < kShort)
                    for (int k = 0; k < npx; k++) push((int)(((int64_t)k * 7919 + (int64_t)s * 104729) % npx), s);
                else
                    for (const int px : longPixels) push(px, s);
            }
            const int64_t n = (int64_t)pixels.size();
            for (Film *f : {&viaArrays, &viaC, &sequential}) {
                void *st = f->est.DeviceStream();
                DeviceArray dPixels(pixels.data(), pixels.size() * sizeof(int32_t), st);
                DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), st), d1(smp[1].data(), smp[1].size() * sizeof(float), st),
                    d2(smp[2].data(), smp[2].size() * sizeof(float), st);
                const int32_t *px = static_cast<const int32_t *>(dPixels.ptr);
                const std::vector<Estimator::RecordSamples> buffers = {{0, 0, static_cast<const float *>(d0.ptr), true},
                                                                       {1, 0, static_cast<const float *>(d1.ptr)},
                                                                       {2, 0, static_cast<const float *>(d2.ptr)}};
                if (f == &viaArrays) {
                    f->est.AccumulateRecords(px, n, buffers, kSplitAbove);
                } else if (f == &sequential) {
                    f->est.AccumulateRecords(px, n, buffers);
                } else {
                    std::vector<statmc_stat_type> types;
                    for (const auto &b : buffers) {
                        statmc_stat_type t = f->est.DeviceStatistics(b.statTypeIndex, b.bounceIndex, b.withPrepass);
                        t.samples = b.d_samples;
                        types.push_back(t);
                    }
                    check(statmc_accumulate_records_split((uint16_t)W, (uint16_t)H, types.data(), (int)types.size(), px, n, kSplitAbove, st));
                }
                check(statmc_synchronize(st));   // before the arrays are freed
            }
            for (Film *f : {&viaQueue, &viaQueueC}) {
                void *st = f->est.DeviceStream();
                DeviceArray dEntries(entries.data(), entries.size() * sizeof(QueueEntry), st);
                if (f == &viaQueue) {
                    f->est.AccumulateRecordsInterleaved(dEntries.ptr, n, layout, fields, kSplitAbove);
                } else {
                    std::vector<statmc_stat_type> types;
                    statmc_record_layout l{};
                    l.stride = layout.stride;
                    l.pixel_offset = layout.pixelOffset;
                    for (const auto &fl : fields) {
                        l.sample_offset[types.size()] = fl.offset;
                        l.sample_format[types.size()] = fl.format;
                        types.push_back(f->est.DeviceStatistics(fl.statTypeIndex, fl.bounceIndex, fl.withPrepass));
                    }
                    check(statmc_accumulate_records_interleaved_split((uint16_t)W, (uint16_t)H, types.data(), (int)types.size(), dEntries.ptr, &l, n,
                                                                      kSplitAbove, st));
                }
                check(statmc_synchronize(st));
            }
        }
        for (Film *f : {&viaArrays, &viaC, &viaQueue, &viaQueueC, &sequential}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        bool ok = true;
        const Estimator &a = viaC.est;
        const char *names[] = {"AccumulateRecords(splitAbove)", "AccumulateRecordsInterleaved(splitAbove)", "statmc_accumulate_records_interleaved_split"};
        const Film *others[] = {&viaArrays, &viaQueue, &viaQueueC};
        for (int k = 0; k < 3; k++) {
            const Estimator &b = others[k]->est;
            auto cmp = [&](const HostImage &x, const HostImage &y, const std::string &what) {
                if (!sameBits(x, y)) {
                    std::printf("MISMATCH %s: %s differs from statmc_accumulate_records_split\n", names[k], what.c_str());
                    ok = false;
                }
            };
            cmp(a.filmFilteredBuffer.mat, b.filmFilteredBuffer.mat, "film-f");
            for (unsigned char i = 0; i < 3; i++) {
                const std::string pre = "t" + std::to_string(i) + "-b0";
                cmp(a.nBuffers[i][0].mat, b.nBuffers[i][0].mat, pre + "-n");
                cmp(a.meanBuffers[i][0].mat, b.meanBuffers[i][0].mat, pre + "-mean");
                cmp(a.m2Buffers[i][0].mat, b.m2Buffers[i][0].mat, pre + "-m2");
                cmp(a.m3Buffers[i][0].mat, b.m3Buffers[i][0].mat, pre + "-m3");
                cmp(a.filmBuffers[i][0].mat, b.filmBuffers[i][0].mat, pre + "-film-mean");
                cmp(a.filmM2Buffers[i][0].mat, b.filmM2Buffers[i][0].mat, pre + "-film-m2");
            }
        }
        const int32_t *n = a.nBuffers[0][0].mat.ptr<int32_t>();
        for (int k = 0; k < npx; k++)
            if (n[k] != fed[k]) {
                std::printf("MISMATCH count %d at pixel %d, fed %d\n", n[k], k, fed[k]);
                ok = false;
                break;
            }
        if (!sameBits(a.nBuffers[0][0].mat, sequential.est.nBuffers[0][0].mat)) {
            std::printf("MISMATCH the sequential entry's counts\n");
            ok = false;
        }
        if (sameBits(a.m2Buffers[0][0].mat, sequential.est.m2Buffers[0][0].mat)) {
            std::printf("MISMATCH the radiance m2 equals the sequential entry's in every bit: nothing was split\n");
            ok = false;
        }
        if (!ok) return 1;
        std::printf("accumulate records split ok: %dx%d, %d long pixels of %d, split above %d\n", W, H, (int)(sizeof(longPixels) / sizeof(int)), 2 * kLong,
                    kSplitAbove);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
