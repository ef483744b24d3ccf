// Estimator::GatherStates and Estimator::CombineRecords against the C entries they stand for and against CombineStatistics.
// Film B holds two samples on every third pixel; three more films hold three samples everywhere.  The list is B's touched pixels in
// a scrambled order with skipped entries in between.
//   1  viaEstimator  B.GatherStates, then CombineRecords (the radiance type with its pre-pass epilogue)
//   2  viaC          statmc_gather_states / statmc_combine_records on the descriptors of DeviceStatistics
//   3  viaDense      CombineStatistics(B): the whole-film combine
// The gathered records of 1 and 2 must be the same bits, a skipped entry's record all zeros; after Upload / Denoise / Download /
// DownloadStatistics every statistics image and "film-f" must be the same bits in 1 and 2, and every statistics image the same
// bits in 3 (whose "film" image is combined too, so its "film-f" is another).  splitAbove = 0 must come back as
// STATMC_ERR_INVALID naming split_above.
//   test_state_records [width height]     prints "state records ok" and exits 0, or names the first difference
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
    size_t bytes;
    explicit DeviceArray(size_t n) : bytes(n) {
        check(statmc_malloc(&ptr, bytes));
        check(statmc_memset(ptr, 0x5a, bytes, nullptr));
        check(statmc_synchronize(nullptr));
    }
    DeviceArray(const void *host, size_t n, void *stream) : bytes(n) {
        check(statmc_malloc(&ptr, bytes));
        check(statmc_upload(ptr, host, bytes, stream));
    }
    ~DeviceArray() { statmc_free(ptr); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    std::vector<int32_t> host(void *stream) const {
        std::vector<int32_t> h(bytes / 4);
        check(statmc_download(h.data(), ptr, bytes, stream));
        check(statmc_synchronize(stream));
        return h;
    }
};

// samples s0 .. s0 + count - 1 of the pixels k with k % every == 0, through AccumulateRecords
void feed(Film &f, int npx, int every, int s0, int count) {
    std::vector<int32_t> pixels;
    std::vector<float> smp[3];
    const int m = (npx + every - 1) / every;      // the multiples of `every` below npx, in an order that depends on s (7919 is prime, m smaller)
    for (int s = s0; s < s0 + count; s++)
        for (int j = 0; j < m; j++) {
            const int px = (int)(((int64_t)j * 7919 + (int64_t)s * 31) % m) * every;
            pixels.push_back(px);
            for (int t = 0; t < 3; t++)
                for (int c = 0; c < 3; c++) smp[t].push_back(sampleOf(t, px, s, c));
        }
    void *st = f.est.DeviceStream();
    DeviceArray dPixels(pixels.data(), pixels.size() * sizeof(int32_t), st);
    DeviceArray d0(smp[0].data(), smp[0].size() * sizeof(float), st), d1(smp[1].data(), smp[1].size() * sizeof(float), st),
        d2(smp[2].data(), smp[2].size() * sizeof(float), st);
    f.est.AccumulateRecords(static_cast<const int32_t *>(dPixels.ptr), (int64_t)pixels.size(),
                            {{0, 0, static_cast<const float *>(d0.ptr)}, {1, 0, static_cast<const float *>(d1.ptr)}, {2, 0, static_cast<const float *>(d2.ptr)}});
    check(statmc_synchronize(st));   // before the arrays are freed
}

}  // namespace

int main(int argc, char **argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 61, H = argc > 2 ? std::atoi(argv[2]) : 37;
    const int npx = W * H;
    if (npx >= 7919 || npx < 130) {
        std::printf("film size not supported by this test\n");
        return 1;
    }
    try {
        StatPathParams p;
        p.denoiseImage = true;   // radiance (RGB, Box-Cox, M3) + normal / albedo G-buffers (RGB, M1)
        const StatTypeConfigs cfgs = makeStatTypeConfigs(p);
        Film source(W, H, cfgs), viaEstimator(W, H, cfgs), viaC(W, H, cfgs), viaDense(W, H, cfgs);
        if (source.est.statTypeConfigs.nEnabled != 3) {
            std::printf("unexpected configuration: %d types\n", source.est.statTypeConfigs.nEnabled);
            return 1;
        }
        const size_t dwords[3] = {statmc_state_dwords(3, 3, 1), statmc_state_dwords(3, 1, 0), statmc_state_dwords(3, 1, 0)};
        if (dwords[0] != 16 || dwords[1] != 4 || dwords[2] != 4) {
            std::printf("statmc_state_dwords: %zu %zu %zu\n", dwords[0], dwords[1], dwords[2]);
            return 1;
        }
        try {
            viaEstimator.est.CombineRecords(nullptr, 0, {}, 0);
            std::printf("splitAbove = 0 was not refused\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != STATMC_ERR_INVALID || std::strstr(e.what(), "split_above") == nullptr) throw;
        }

        feed(source, npx, 3, 500, 2);
        for (Film *f : {&viaEstimator, &viaC, &viaDense}) feed(*f, npx, 1, 0, 3);

        // the list: the source's touched pixels, scrambled (104729 is prime), every seventh entry a skipped one
        std::vector<int32_t> list;
        const int touched = (npx + 2) / 3;
        for (int j = 0; j < touched; j++) {
            if (list.size() % 7 == 3) list.push_back(list.size() % 2 ? -1 : npx + 7);
            list.push_back((int32_t)((((int64_t)j * 104729) % touched) * 3));
        }
        const int64_t n = (int64_t)list.size();
        void *srcStream = source.est.DeviceStream();
        DeviceArray dList(list.data(), list.size() * sizeof(int32_t), srcStream);
        const int32_t *dPx = static_cast<const int32_t *>(dList.ptr);
        DeviceArray e0(n * dwords[0] * 4), e1(n * dwords[1] * 4), e2(n * dwords[2] * 4), c0(n * dwords[0] * 4), c1(n * dwords[1] * 4), c2(n * dwords[2] * 4);
        source.est.GatherStates(dPx, n, {{0, 0, e0.ptr}, {1, 0, e1.ptr}, {2, 0, e2.ptr}});
        {
            std::vector<statmc_stat_type> types;
            for (unsigned char i = 0; i < 3; i++) types.push_back(source.est.DeviceStatistics(i, 0));
            void *states[3] = {c0.ptr, c1.ptr, c2.ptr};
            check(statmc_gather_states((uint16_t)W, (uint16_t)H, types.data(), 3, dPx, n, states, srcStream));
        }
        check(statmc_synchronize(srcStream));
        bool ok = true;
        const DeviceArray *viaE[3] = {&e0, &e1, &e2}, *viaS[3] = {&c0, &c1, &c2};
        for (int t = 0; t < 3; t++) {
            const std::vector<int32_t> a = viaE[t]->host(srcStream), b = viaS[t]->host(srcStream);
            if (a != b) {
                std::printf("MISMATCH GatherStates: the records of type %d differ from statmc_gather_states\n", t);
                ok = false;
            }
            for (int64_t i = 0; i < n && ok; i++) {
                const bool dead = list[i] < 0 || list[i] >= npx;
                const int32_t want = dead ? 0 : 2;     // two samples per touched pixel
                if (a[i * dwords[t]] != want) {
                    std::printf("MISMATCH GatherStates: record %lld of type %d has count %d, expected %d\n", (long long)i, t, a[i * dwords[t]], want);
                    ok = false;
                }
                for (size_t d = 0; dead && d < dwords[t]; d++)
                    if (a[i * dwords[t] + d] != 0) {
                        std::printf("MISMATCH GatherStates: a skipped entry's record is not all zeros (type %d)\n", t);
                        ok = false;
                        break;
                    }
            }
        }

        {
            void *st = viaEstimator.est.DeviceStream();
            DeviceArray dHere(list.data(), list.size() * sizeof(int32_t), st);
            viaEstimator.est.CombineRecords(static_cast<const int32_t *>(dHere.ptr), n, {{0, 0, e0.ptr, true}, {1, 0, e1.ptr}, {2, 0, e2.ptr}});
            check(statmc_synchronize(st));
        }
        {
            void *st = viaC.est.DeviceStream();
            DeviceArray dHere(list.data(), list.size() * sizeof(int32_t), st);
            std::vector<statmc_stat_type> types;
            for (unsigned char i = 0; i < 3; i++) types.push_back(viaC.est.DeviceStatistics(i, 0, i == 0));
            const void *states[3] = {c0.ptr, c1.ptr, c2.ptr};
            check(statmc_combine_records((uint16_t)W, (uint16_t)H, types.data(), 3, static_cast<const int32_t *>(dHere.ptr), n, states, INT32_MAX, st));
            check(statmc_synchronize(st));
        }
        viaDense.est.CombineStatistics(source.est);

        for (Film *f : {&viaEstimator, &viaC, &viaDense}) {
            f->est.Upload();
            f->est.Denoise();
            f->est.Download();
            f->est.DownloadStatistics();
            f->est.Synchronize();
        }
        const Estimator &a = viaC.est;
        const char *names[] = {"GatherStates / CombineRecords", "CombineStatistics"};
        const Film *others[] = {&viaEstimator, &viaDense};
        for (int k = 0; k < 2; k++) {
            const Estimator &b = others[k]->est;
            auto cmp = [&](const HostImage &x, const HostImage &y, const std::string &what) {
                if (!sameBits(x, y)) {
                    std::printf("MISMATCH %s: %s differs from statmc_gather_states / statmc_combine_records\n", names[k], what.c_str());
                    ok = false;
                }
            };
            if (k == 0) cmp(a.filmFilteredBuffer.mat, b.filmFilteredBuffer.mat, "film-f");
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
        const int32_t *cnt = a.nBuffers[0][0].mat.ptr<int32_t>();
        for (int k = 0; k < npx; k++)
            if (cnt[k] != (k % 3 == 0 ? 5 : 3)) {
                std::printf("MISMATCH count %d at pixel %d\n", cnt[k], k);
                ok = false;
                break;
            }
        if (!ok) return 1;
        std::printf("state records ok: %dx%d, %lld records\n", W, H, (long long)n);
        return 0;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
