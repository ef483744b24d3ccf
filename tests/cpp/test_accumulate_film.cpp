// An Estimator fed through Estimator::AccumulateFilm -- whole-film sample arenas in the format the renderer holds them in: the
// radiance type fp32, the normal and albedo G-buffers IEEE half -- against one filled through StatTile recorders and Merge*Tile
// flushes with the same samples widened to fp32: after Upload / Denoise / Download / DownloadStatistics the "film-f" image and
// every statistics image must be the same bits.  Two batches, so the second starts from n > 0; an odd film size; the radiance
// type is folded with its pre-pass epilogue, which Denoise() recomputes.
//   test_accumulate_film [width height]       prints "accumulate film OK" and exits 0, or names the first difference
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
// sample s of pixel (x, y), channel c of stat type `type`: positive radiance with the odd firefly; features k / 2048 in [0, 1),
// values a half holds exactly
float sampleOf(int type, int x, int y, int s, int c, int width) {
    const uint32_t h = mix32((uint32_t)(y * width + x) * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    if (type != 0) return (float)(h >> 21) * (1.f / 2048.f);
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.01f + u * u);
}
// the binary16 pattern of a value that is a normal half or zero, exactly (anything else: the test's own mistake)
uint16_t halfBits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) == 0) return (uint16_t)(u >> 16);
    const int e = (int)((u >> 23) & 255) - 127 + 15;
    if (e < 1 || e > 30 || (u & 0x1fffu) != 0) {
        std::printf("halfBits: %g is no normal half\n", v);
        std::exit(1);
    }
    return (uint16_t)(((u >> 16) & 0x8000u) | ((uint32_t)e << 10) | ((u >> 13) & 0x3ffu));
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
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film merged(W, H, cfgs), arenas(W, H, cfgs);
        const auto &kept = merged.est.statTypeConfigs;
        if (kept.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", kept.nEnabled);
            return 1;
        }
        try {   // the statistics must live on the device first
            arenas.est.AccumulateFilm(0, {{0, 0, nullptr, STATMC_SAMPLES_F32}});
            std::printf("AccumulateFilm before EnableDeviceAccumulation did not throw\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID) throw;
        }
        merged.est.EnableDeviceAccumulation((size_t)64 << 20);
        arenas.est.EnableDeviceAccumulation((size_t)64 << 20);

        int s0 = 0;
        for (const int S : batches) {
            // ---- Merge*Tile: 16 x 16 tiles record the (widened) samples, the flush runs statmc_accumulate_tiles
            for (int ty = 0; ty < H; ty += 16)
                for (int tx = 0; tx < W; tx += 16) {
                    const Bounds2i b(Point2i(tx, ty), Point2i(std::min(tx + 16, W), std::min(ty + 16, H)));
                    auto tiles = merged.est.GetTiles<Vec3>(b, 1, (unsigned char)kept.nEnabled);   // [bounce][type]
                    for (int y = b.pMin.y; y < b.pMax.y; y++)
                        for (int x = b.pMin.x; x < b.pMax.x; x++)
                            for (int s = s0; s < s0 + S; s++)
                                for (int i = 0; i < kept.nEnabled; i++) {
                                    const Vec3 v{sampleOf(i, x, y, s, 0, W), sampleOf(i, x, y, s, 1, W), sampleOf(i, x, y, s, 2, W)};
                                    if (i == 0) tiles[0][i].AddTransformSampleM3(Point2i(x, y), v);
                                    else tiles[0][i].AddSampleM1(Point2i(x, y), v);
                                }
                    merged.est.MergeTransformTile(tiles[0][0], 0, 0);
                    for (unsigned char i = 1; i < kept.nEnabled; i++) merged.est.MergeTile(tiles[0][i], i, 0);
                }
            merged.est.FlushSamples();
            // ---- the film-major arenas [S][H][W][3]: radiance fp32, the two G-buffers half
            std::vector<float> rad;
            std::vector<uint16_t> feat[2];
            for (int s = s0; s < s0 + S; s++)
                for (int k = 0; k < npx; k++)
                    for (int c = 0; c < 3; c++) {
                        rad.push_back(sampleOf(0, k % W, k / W, s, c, W));
                        for (int i = 1; i < 3; i++) feat[i - 1].push_back(halfBits(sampleOf(i, k % W, k / W, s, c, W)));
                    }
            void *st = arenas.est.DeviceStream();
            DeviceArray d0(rad.data(), rad.size() * sizeof(float), st), d1(feat[0].data(), feat[0].size() * sizeof(uint16_t), st),
                d2(feat[1].data(), feat[1].size() * sizeof(uint16_t), st);
            arenas.est.AccumulateFilm(S, {{0, 0, d0.ptr, STATMC_SAMPLES_F32, true},
                                          {1, 0, d1.ptr, STATMC_SAMPLES_F16},
                                          {2, 0, d2.ptr, STATMC_SAMPLES_F16}});
            check(statmc_synchronize(st));   // before the arrays are freed
            s0 += S;
        }
        for (Film *f : {&merged, &arenas}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        bool ok = sameBits(merged.est.filmFilteredBuffer.mat, arenas.est.filmFilteredBuffer.mat, "film-f");
        const Estimator &a = merged.est, &b = arenas.est;
        for (unsigned char i = 0; i < kept.nEnabled; i++) {
            const std::string pre = "t" + std::to_string(i) + "-b0";
            ok &= sameBits(a.nBuffers[i][0].mat, b.nBuffers[i][0].mat, pre + "-n");
            ok &= sameBits(a.meanBuffers[i][0].mat, b.meanBuffers[i][0].mat, pre + "-mean");
            ok &= sameBits(a.m2Buffers[i][0].mat, b.m2Buffers[i][0].mat, pre + "-m2");
            ok &= sameBits(a.m3Buffers[i][0].mat, b.m3Buffers[i][0].mat, pre + "-m3");
            ok &= sameBits(a.filmBuffers[i][0].mat, b.filmBuffers[i][0].mat, pre + "-film-mean");
            ok &= sameBits(a.filmM2Buffers[i][0].mat, b.filmM2Buffers[i][0].mat, pre + "-film-m2");
        }
        const int32_t *n = b.nBuffers[0][0].mat.ptr<int32_t>();
        for (int k = 0; k < npx; k++)
            if (n[k] != batches[0] + batches[1]) {
                std::printf("MISMATCH count %d at pixel %d\n", n[k], k);
                ok = false;
                break;
            }
        if (!ok) return 1;
        std::printf("accumulate film OK: %dx%d, %d + %d samples, %d types\n", W, H, batches[0], batches[1], kept.nEnabled);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
