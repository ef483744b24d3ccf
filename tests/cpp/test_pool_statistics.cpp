// Estimator::PoolStatistics: a fine Estimator whose statistics live on the device (AccumulateFilm with per-pixel counts, whole
// blocks without a sample included) pooled k x k into a coarse Estimator, which is then denoised and downloaded like any other.
// Against the C entry called by hand on the same device images: every statistics image, the counts and the "film" image of the
// coarse Estimator must be the bits statmc_pool_statistics leaves, and coarse.Denoise() must leave the "film-f" of a third
// Estimator of the coarse size that is given those pooled images from the host and goes through Upload / Denoise / Download.
//   test_pool_statistics [width height k]       prints "pool statistics OK" and exits 0, or names the first difference
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
// sample s of pixel (x, y), channel c of stat type `type`: positive radiance with the odd firefly; features in [0, 1)
float sampleOf(int type, int x, int y, int s, int c, int width) {
    const uint32_t h = mix32((uint32_t)(y * width + x) * 0x9e3779b9u ^ mix32((uint32_t)(s * 8 + type * 3 + c) + 0x632be5abu));
    if (type != 0) return (float)(h >> 21) * (1.f / 2048.f);
    const float u = (float)(h >> 8) * (1.f / 16777216.f);
    return ((h & 63u) == 0 ? 50.f : 1.f) * (0.01f + u * u);
}

struct Film {
    Buffer film;
    BufferRegistry reg;
    Estimator est;
    Film(int w, int h, const StatTypeConfigs &cfgs)
        : film("film", HostImage(h, w, F32C3)), reg(film),
          est(film, cfgs, 10.f, 20, /*denoiseFilm=*/true, /*acrr=*/false, /*smis=*/false, reg) {
        float *f = film.mat.ptr<float>();
        for (int i = 0; i < w * h * 3; i++) f[i] = sampleOf(0, (i / 3) % w, (i / 3) / w, 1000, i % 3, w);
        est.AllocateBuffers(reg);
    }
};

struct DeviceArray {
    void *ptr = nullptr;
    size_t bytes;
    explicit DeviceArray(size_t bytes) : bytes(bytes) { check(statmc_malloc(&ptr, bytes)); }
    DeviceArray(const void *host, size_t bytes, void *stream) : DeviceArray(bytes) { check(statmc_upload(ptr, host, bytes, stream)); }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    std::vector<char> host(void *stream) const {
        std::vector<char> v(bytes);
        check(statmc_download(v.data(), ptr, bytes, stream));
        check(statmc_synchronize(stream));
        return v;
    }
};

bool sameBytes(const void *a, const void *b, size_t bytes, const std::string &what) {
    if (std::memcmp(a, b, bytes) != 0) {
        std::printf("MISMATCH %s\n", what.c_str());
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const int W = argc > 3 ? std::atoi(argv[1]) : 37, H = argc > 3 ? std::atoi(argv[2]) : 23, K = argc > 3 ? std::atoi(argv[3]) : 4;
    const int S = 9, npx = W * H, Wc = (W + K - 1) / K, Hc = (H + K - 1) / K, ncx = Wc * Hc;
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film fine(W, H, cfgs), coarse(Wc, Hc, cfgs), fromHost(Wc, Hc, cfgs), wrongSize(Wc + 1, Hc, cfgs);
        Estimator &f = fine.est, &c = coarse.est;
        const int nTypes = f.statTypeConfigs.nEnabled;
        if (nTypes != 3) {
            std::printf("unexpected configuration: %d types\n", nTypes);
            return 1;
        }
        f.EnableDeviceAccumulation((size_t)64 << 20);
        // ---- the fine film: 0 .. S samples per pixel, the block at the origin and every fifth pixel without any
        std::vector<int32_t> counts(npx);
        for (int k = 0; k < npx; k++) {
            const int x = k % W, y = k / W;
            counts[k] = (x < K && y < K) || k % 5 == 0 ? 0 : (int)(mix32((uint32_t)k + 77u) % (uint32_t)(S + 1));
        }
        std::vector<float> arena[3];
        for (int s = 0; s < S; s++)
            for (int k = 0; k < npx; k++)
                for (int ch = 0; ch < 3; ch++)
                    for (int i = 0; i < 3; i++) arena[i].push_back(sampleOf(i, k % W, k / W, s, ch, W));
        void *st = f.DeviceStream();
        {
            DeviceArray d0(arena[0].data(), arena[0].size() * 4, st), d1(arena[1].data(), arena[1].size() * 4, st),
                d2(arena[2].data(), arena[2].size() * 4, st), dc(counts.data(), counts.size() * 4, st);
            f.AccumulateFilm(S, {{0, 0, d0.ptr, STATMC_SAMPLES_F32}, {1, 0, d1.ptr, STATMC_SAMPLES_F32}, {2, 0, d2.ptr, STATMC_SAMPLES_F32}},
                             static_cast<const int32_t *>(dc.ptr));
            check(statmc_synchronize(st));   // before the arrays are freed
        }
        f.Upload();   // the "film" image

        // ---- what the wrapper refuses
        int refused = 0;
        for (int bad = 0; bad < 4; bad++) {
            try {
                if (bad == 0) f.PoolStatistics(c, 3);
                if (bad == 1) f.PoolStatistics(f, K);
                if (bad == 2) f.PoolStatistics(wrongSize.est, K);
                if (bad == 3) f.PoolStatistics(c, K, {0});
            } catch (const Error &e) {
                if (e.code != STATMC_ERR_INVALID) throw;
                refused++;
            }
        }
        if (refused != 4) {
            std::printf("PoolStatistics refused %d of 4 invalid calls\n", refused);
            return 1;
        }

        // ---- the Estimator's way
        f.PoolStatistics(c, K);
        c.Denoise();
        c.Download();
        c.DownloadStatistics();
        c.Synchronize();
        const std::vector<char> pooledFilm = [&] {
            std::vector<char> v((size_t)ncx * 12);
            check(statmc_download(v.data(), c.filmBuffer.gpuMat.data(), v.size(), c.DeviceStream()));
            check(statmc_synchronize(c.DeviceStream()));
            return v;
        }();

        // ---- the C entry by hand on the fine Estimator's device images
        f.Synchronize();
        std::vector<std::unique_ptr<DeviceArray>> imgs;
        auto image = [&](size_t bytes) {
            imgs.emplace_back(new DeviceArray(bytes));
            check(statmc_memset(imgs.back()->ptr, 0xff, bytes, st));
            return imgs.back().get();
        };
        struct Out { DeviceArray *n, *mean, *m2, *m3, *fm, *fm2; };
        std::vector<Out> outs;
        std::vector<statmc_pool_entry> entries;
        for (unsigned char i = 0; i < nTypes; i++) {
            const auto &cfg = f.statTypeConfigs[i];
            const size_t img = (size_t)ncx * cfg.nChannels * 4;
            Out o{image((size_t)ncx * 4), image(img), image(img), image(img), nullptr, nullptr};
            statmc_pool_entry e;
            std::memset(&e, 0, sizeof(e));
            e.count_of = -1;
            e.dst.channels = e.src.channels = cfg.nChannels;
            e.dst.max_moment = e.src.max_moment = cfg.maxMoment;
            e.src.n = static_cast<int32_t *>(f.nBuffers[i][0].gpuMat.data());
            e.src.mean = static_cast<float *>(f.meanBuffers[i][0].gpuMat.data());
            e.src.m2 = static_cast<float *>(f.m2Buffers[i][0].gpuMat.data());
            e.src.m3 = static_cast<float *>(f.m3Buffers[i][0].gpuMat.data());
            e.dst.n = static_cast<int32_t *>(o.n->ptr);
            e.dst.mean = static_cast<float *>(o.mean->ptr);
            e.dst.m2 = static_cast<float *>(o.m2->ptr);
            e.dst.m3 = static_cast<float *>(o.m3->ptr);
            if (cfg.transform) {
                o.fm = image(img), o.fm2 = image(img);
                e.src.film_mean = static_cast<float *>(f.filmBuffers[i][0].gpuMat.data());
                e.src.film_m2 = static_cast<float *>(f.filmM2Buffers[i][0].gpuMat.data());
                e.dst.film_mean = static_cast<float *>(o.fm->ptr);
                e.dst.film_m2 = static_cast<float *>(o.fm2->ptr);
            }
            outs.push_back(o);
            entries.push_back(e);
        }
        DeviceArray *byHandFilm = image((size_t)ncx * 12);
        {
            statmc_pool_entry e;
            std::memset(&e, 0, sizeof(e));
            e.count_of = 0;
            e.dst.channels = e.src.channels = 3;
            e.dst.max_moment = e.src.max_moment = 1;
            e.src.mean = static_cast<float *>(f.filmBuffer.gpuMat.data());
            e.dst.mean = static_cast<float *>(byHandFilm->ptr);
            entries.push_back(e);
        }
        check(statmc_pool_statistics((uint16_t)W, (uint16_t)H, K, entries.data(), (int)entries.size(), st));

        bool ok = true;
        long long total = 0;
        for (unsigned char i = 0; i < nTypes; i++) {
            const auto &cfg = f.statTypeConfigs[i];
            const std::string pre = "t" + std::to_string(i) + "-b0";
            const Out &o = outs[i];
            Film &h = fromHost;
            auto both = [&](DeviceArray *mine, Buffer &theirs, Buffer &upload, const std::string &what) {
                const std::vector<char> v = mine->host(st);
                ok &= v.size() == theirs.mat.bytes() && sameBytes(v.data(), theirs.mat.ptr(), v.size(), pre + what);
                std::memcpy(upload.mat.ptr(), v.data(), v.size());
            };
            both(o.n, c.nBuffers[i][0], h.est.nBuffers[i][0], "-n");
            both(o.mean, c.meanBuffers[i][0], h.est.meanBuffers[i][0], "-mean");
            if (cfg.maxMoment >= 2) both(o.m2, c.m2Buffers[i][0], h.est.m2Buffers[i][0], "-m2");
            if (cfg.maxMoment >= 3) both(o.m3, c.m3Buffers[i][0], h.est.m3Buffers[i][0], "-m3");
            if (cfg.transform) {
                both(o.fm, c.filmBuffers[i][0], h.est.filmBuffers[i][0], "-film-mean");
                both(o.fm2, c.filmM2Buffers[i][0], h.est.filmM2Buffers[i][0], "-film-m2");
            }
            if (i == 0) {
                const int32_t *n = c.nBuffers[0][0].mat.ptr<int32_t>();
                for (int Y = 0; Y < Hc; Y++)
                    for (int X = 0; X < Wc; X++) {
                        int sum = 0;
                        for (int y = Y * K; y < std::min((Y + 1) * K, H); y++)
                            for (int x = X * K; x < std::min((X + 1) * K, W); x++) sum += counts[y * W + x];
                        if (n[Y * Wc + X] != sum) {
                            std::printf("MISMATCH count %d at coarse pixel (%d, %d): the block holds %d samples\n", n[Y * Wc + X], X, Y, sum);
                            return 1;
                        }
                        total += sum;
                    }
                if (n[0] != 0) {
                    std::printf("the block at the origin should be empty\n");
                    return 1;
                }
            }
        }
        const std::vector<char> film = byHandFilm->host(st);
        ok &= sameBytes(film.data(), pooledFilm.data(), film.size(), "film");
        std::memcpy(fromHost.est.filmBuffer.mat.ptr(), film.data(), film.size());

        // ---- the pooled images from the host through Upload / Denoise / Download
        fromHost.est.Upload();
        fromHost.est.Denoise();
        fromHost.est.Download();
        fromHost.est.Synchronize();
        ok &= sameBytes(fromHost.est.filmFilteredBuffer.mat.ptr(), c.filmFilteredBuffer.mat.ptr(), c.filmFilteredBuffer.mat.bytes(), "film-f");
        const float *ff = c.filmFilteredBuffer.mat.ptr<float>();
        bool nonzero = false;
        for (int k = 0; k < ncx * 3; k++) nonzero |= ff[k] != 0.f;
        if (!nonzero) {
            std::printf("film-f of the coarse film is all zeros\n");
            return 1;
        }
        if (!ok) return 1;
        std::printf("pool statistics OK: %dx%d -> %dx%d (k = %d), %lld samples, %d types\n", W, H, Wc, Hc, K, total, nTypes);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
