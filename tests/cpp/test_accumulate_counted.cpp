// Per-pixel sample budgets through the C++ host: an Estimator fed RAGGED StatTiles -- every pixel of a tile with its own number
// of samples -- through Merge[Transform]Tile(s), against one fed the same samples, ordered by sample index, through
// Estimator::AccumulateRecords, and one fed the dense arena plus the count image through Estimator::AccumulateFilm(nSamples,
// buffers, d_counts).  After Upload / Denoise / Download / DownloadStatistics the "film-f" image and every statistics image must
// be the same bits in all three.  Three batches: ragged, uniform (its flush must stage no counts: today's calls, today's bits),
// ragged again on the state the first two left; an odd film size; pixels and whole tile edges without any sample.
//   test_accumulate_counted [width height]       prints "accumulate counted ok" and exits 0, or names the first difference
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
// sample s of pixel (x, y), channel c of stat type `type`: positive radiance with the odd firefly, features in [0, 1)
float sampleOf(int type, int x, int y, int s, int c, int width) {
    const uint32_t h = mix32((uint32_t)(y * width + x) * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    if (type != 0) return u;
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.01f + u * u);
}
// the budget of pixel (x, y) in batch b: `cap` everywhere in a uniform batch; otherwise 0 .. cap, about a quarter of the pixels and
// the first column and last row of every 16 x 16 tile at 0 (the slot is then smaller than the tile)
int budgetOf(int b, int x, int y, int cap, bool uniform) {
    if (uniform) return cap;
    if (x % 16 == 0 || y % 16 == 15) return 0;
    const uint32_t h = mix32((uint32_t)(x * 131 + y * 7 + b * 977));
    return (h & 3u) == 0 ? 0 : (int)(h >> 8) % (cap + 1);
}

struct Film {
    Buffer film;
    BufferRegistry reg;
    Estimator est;
    Film(int w, int h, const StatTypeConfigs &cfgs)
        : film("film", HostImage(h, w, F32C3)), reg(film),
          est(film, cfgs, 10.f, 20, /*denoiseFilm=*/true, /*acrr=*/false, /*smis=*/false, reg) {
        float *f = film.mat.ptr<float>();
        for (int i = 0; i < w * h * 3; i++) f[i] = sampleOf(0, i % w, i / w, 1000, i % 3, w);
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
        check(statmc_malloc(&ptr, bytes ? bytes : 4));
        if (bytes) check(statmc_upload(ptr, host, bytes, stream));
    }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
};

}  // namespace

int main(int argc, char **argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 61, H = argc > 2 ? std::atoi(argv[2]) : 37;
    struct Batch { int cap; bool uniform; };
    const Batch batches[3] = {{6, false}, {4, true}, {9, false}};
    const int npx = W * H;
    if (npx % 7919 == 0) {   // the records visit the pixels in the order k -> (7919 k + ...) mod npx: a permutation otherwise
        std::printf("film size not supported by this test's pixel permutation\n");
        return 1;
    }
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film merged(W, H, cfgs), records(W, H, cfgs), arena(W, H, cfgs);
        const auto &kept = merged.est.statTypeConfigs;
        if (kept.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", kept.nEnabled);
            return 1;
        }
        for (Film *f : {&merged, &records, &arena}) f->est.EnableDeviceAccumulation((size_t)64 << 20);

        std::vector<int> fed(npx, 0);
        int s0 = 0;
        for (int b = 0; b < 3; b++) {
            const int cap = batches[b].cap;
            auto budget = [&](int x, int y) { return budgetOf(b, x, y, cap, batches[b].uniform); };
            // ---- Merge*Tile(s): 16 x 16 tiles record every pixel's samples; the flush of a ragged batch takes the counted entry
            const size_t countedBefore = merged.est.countedFlushes();
            for (int ty = 0; ty < H; ty += 16)
                for (int tx = 0; tx < W; tx += 16) {
                    const Bounds2i tb(Point2i(tx, ty), Point2i(std::min(tx + 16, W), std::min(ty + 16, H)));
                    auto lT = merged.est.GetTiles<Vec3>(tb, 1);
                    auto fT = merged.est.GetTiles<Vec3>(tb, 1, 2);
                    for (int y = tb.pMin.y; y < tb.pMax.y; y++)
                        for (int x = tb.pMin.x; x < tb.pMax.x; x++)
                            for (int s = 0; s < budget(x, y); s++) {
                                auto v = [&](int i) { return Vec3{sampleOf(i, x, y, s0 + s, 0, W), sampleOf(i, x, y, s0 + s, 1, W), sampleOf(i, x, y, s0 + s, 2, W)}; };
                                lT[0].AddTransformSampleM3(Point2i(x, y), v(0));
                                fT[0][0].AddSampleM1(Point2i(x, y), v(1));
                                fT[0][1].AddSampleM1(Point2i(x, y), v(2));
                            }
                    merged.est.MergeTransformTiles(lT, cfgs[Radiance]);
                    merged.est.MergeTiles(fT, std::vector<StatTypeConfig>{cfgs[StatNormal], cfgs[StatAlbedo]});
                }
            merged.est.FlushSamples();
            if (merged.est.countedFlushes() - countedBefore != (batches[b].uniform ? 0u : 1u)) {
                std::printf("batch %d: %zu counted flushes\n", b, merged.est.countedFlushes() - countedBefore);
                return 1;
            }
            // ---- the same samples as records ordered by s, the pixels in an order that depends on s
            std::vector<int32_t> pixels;
            std::vector<float> smp[3];
            for (int s = 0; s < cap; s++)
                for (int k = 0; k < npx; k++) {
                    const int px = (int)(((int64_t)k * 7919 + (int64_t)s * 104729) % npx);
                    if (s >= budget(px % W, px / W)) continue;
                    pixels.push_back(px);
                    for (int i = 0; i < 3; i++)
                        for (int c = 0; c < 3; c++) smp[i].push_back(sampleOf(i, px % W, px / W, s0 + s, c, W));
                }
            {
                void *st = records.est.DeviceStream();
                DeviceArray dPixels(pixels.data(), pixels.size() * sizeof(int32_t), st);
                DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), st), d1(smp[1].data(), smp[1].size() * sizeof(float), st),
                    d2(smp[2].data(), smp[2].size() * sizeof(float), st);
                records.est.AccumulateRecords(static_cast<const int32_t *>(dPixels.ptr), (int64_t)pixels.size(),
                                              {{0, 0, static_cast<const float *>(d0.ptr)},
                                               {1, 0, static_cast<const float *>(d1.ptr)},
                                               {2, 0, static_cast<const float *>(d2.ptr)}});
                check(statmc_synchronize(st));   // before the arrays are freed
            }
            // ---- the dense arena [cap][H][W][3] (dead slots NaN) and the count image, some counts outside [0, cap]
            {
                std::vector<int32_t> counts(npx);
                std::vector<float> dense[3];
                for (auto &d : dense) d.assign((size_t)cap * npx * 3, std::numeric_limits<float>::quiet_NaN());
                for (int k = 0; k < npx; k++) {
                    const int c = budget(k % W, k / W);
                    counts[k] = c == cap && k % 3 == 0 ? cap + 5 : c == 0 && k % 2 == 0 ? -4 : c;
                    for (int s = 0; s < c; s++)
                        for (int i = 0; i < 3; i++)
                            for (int ch = 0; ch < 3; ch++) dense[i][((size_t)s * npx + k) * 3 + ch] = sampleOf(i, k % W, k / W, s0 + s, ch, W);
                }
                void *st = arena.est.DeviceStream();
                DeviceArray dCounts(counts.data(), counts.size() * sizeof(int32_t), st);
                DeviceArray d0(dense[0].data(), dense[0].size() * sizeof(float), st), d1(dense[1].data(), dense[1].size() * sizeof(float), st),
                    d2(dense[2].data(), dense[2].size() * sizeof(float), st);
                arena.est.AccumulateFilm(cap, {{0, 0, d0.ptr, STATMC_SAMPLES_F32}, {1, 0, d1.ptr, STATMC_SAMPLES_F32}, {2, 0, d2.ptr, STATMC_SAMPLES_F32}},
                                         static_cast<const int32_t *>(dCounts.ptr));
                check(statmc_synchronize(st));
            }
            for (int k = 0; k < npx; k++) fed[k] += budget(k % W, k / W);
            s0 += cap;
        }
        for (Film *f : {&merged, &records, &arena}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        bool ok = true;
        const Estimator &a = merged.est;
        for (const Film *f : {&records, &arena}) {
            const Estimator &o = f->est;
            const std::string who = f == &records ? "records: " : "arena: ";
            ok &= sameBits(a.filmFilteredBuffer.mat, o.filmFilteredBuffer.mat, who + "film-f");
            for (unsigned char i = 0; i < kept.nEnabled; i++) {
                const std::string pre = who + "t" + std::to_string(i) + "-b0";
                ok &= sameBits(a.nBuffers[i][0].mat, o.nBuffers[i][0].mat, pre + "-n");
                ok &= sameBits(a.meanBuffers[i][0].mat, o.meanBuffers[i][0].mat, pre + "-mean");
                ok &= sameBits(a.m2Buffers[i][0].mat, o.m2Buffers[i][0].mat, pre + "-m2");
                ok &= sameBits(a.m3Buffers[i][0].mat, o.m3Buffers[i][0].mat, pre + "-m3");
                ok &= sameBits(a.filmBuffers[i][0].mat, o.filmBuffers[i][0].mat, pre + "-film-mean");
                ok &= sameBits(a.filmM2Buffers[i][0].mat, o.filmM2Buffers[i][0].mat, pre + "-film-m2");
            }
        }
        // the counts are what was fed, and no moment took a dead slot's NaN
        const int32_t *n = a.nBuffers[0][0].mat.ptr<int32_t>();
        const float *mean = arena.est.meanBuffers[0][0].mat.ptr<float>();
        for (int k = 0; k < npx && ok; k++) {
            if (n[k] != fed[k]) {
                std::printf("MISMATCH count %d at pixel %d, fed %d\n", n[k], k, fed[k]);
                ok = false;
            }
            if (std::isnan(mean[3 * k])) {
                std::printf("NaN mean at pixel %d\n", k);
                ok = false;
            }
        }
        if (!ok) return 1;
        std::printf("accumulate counted ok: %dx%d, %zu counted of %zu flushes\n", W, H, merged.est.countedFlushes(), merged.est.flushes());
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
