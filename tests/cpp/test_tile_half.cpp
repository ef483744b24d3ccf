// CPU-only checks of the IEEE-half staging of the tile feed (include/statmc_denoiser.hpp), driven by
// tests/test_accumulate_tiles_half_cpu.py.  Links against libstatmc_hip.so only for the symbols; nothing here touches a GPU.
//   test_tile_half convert <in> <out>   <in>: fp32 bit patterns (uint32, native order); <out>: floatToHalfBits of each (uint16)
//   test_tile_half staging              Estimator::SetSampleFormat, the staging's size, counters and contents in a dry run
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "statmc_denoiser.hpp"

using namespace statmc;

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

// the Estimator's staging, through the friend it names for tests
namespace statmc {
struct EstimatorTestAccess {
    static int64_t capacity(const Estimator &e) { return e.acc.capacity; }   // pixel-samples per arena between two flushes
    // the host staging of (statTypeIndex, bounceIndex): floats or 16-bit words by the type's format
    static const void *staged(const Estimator &e, unsigned char ti, unsigned char bj) { return e.acc.arenas.at(ti).at(bj).host.ptr; }
};
}  // namespace statmc

template <class F>
static bool throwsError(F f, int code) {
    try {
        f();
    } catch (const Error &e) {
        return e.code == code;
    }
    return false;
}

static int convert(const char *in, const char *out) {
    FILE *f = std::fopen(in, "rb");
    REQUIRE(f);
    std::vector<uint32_t> bits;
    uint32_t buf[4096];
    for (size_t n; (n = std::fread(buf, 4, 4096, f)) > 0;) bits.insert(bits.end(), buf, buf + n);
    std::fclose(f);
    std::vector<uint16_t> half(bits.size());
    for (size_t i = 0; i < bits.size(); i++) {
        float v;
        std::memcpy(&v, &bits[i], 4);
        half[i] = floatToHalfBits(v);
    }
    f = std::fopen(out, "wb");
    REQUIRE(f);
    REQUIRE(std::fwrite(half.data(), 2, half.size(), f) == half.size());
    std::fclose(f);
    std::printf("converted %zu\n", half.size());
    return 0;
}

// a sample that needs rounding in every channel, different for every (pixel, sample, channel)
static Vec3 sampleAt(int x, int y, int s, float scale) {
    const float v = scale * (1.0f + 0.001f * (float)(x + 37 * y) + 0.3331f * (float)s);
    return Vec3{v, -v * 1.0009765f, v * 3.1415927e-6f};
}

struct Film {
    Film(int w, int h)
        : cfgs(makeStatTypeConfigs(params())), film("film", HostImage(h, w, F32C3), false), reg(film),
          est(film, cfgs, 10.f, 20, false, false, false, reg, false) {
        est.AllocateBuffers(reg);
    }
    static StatPathParams params() {
        StatPathParams p;
        p.denoiseImage = true;   // radiance + normal + albedo: 9 channels
        return p;
    }
    StatTypeConfigs cfgs;
    Buffer film;
    BufferRegistry reg;
    Estimator est;
};

static int staging() {
    const int W = 48, H = 40;
    const size_t budget = (size_t)1 << 20;
    Film f32(W, H), f16(W, H);
    const unsigned char rad = f16.cfgs[Radiance].index, nrm = f16.cfgs[StatNormal].index, alb = f16.cfgs[StatAlbedo].index;
    REQUIRE(throwsError([&] { f16.est.SetSampleFormat(nrm, 2); }, STATMC_ERR_INVALID));
    REQUIRE(throwsError([&] { f16.est.SetSampleFormat(200, STATMC_SAMPLES_F16); }, STATMC_ERR_INVALID));
    f16.est.SetSampleFormat(nrm, STATMC_SAMPLES_F16);
    f16.est.SetSampleFormat(alb, STATMC_SAMPLES_F16);
    f16.est.SetSampleFormat(alb, STATMC_SAMPLES_F32);     // may be changed until the staging is sized
    f16.est.SetSampleFormat(alb, STATMC_SAMPLES_F16);
    f32.est.EnableDeviceAccumulation(budget, /*dryRun=*/true);
    f16.est.EnableDeviceAccumulation(budget, /*dryRun=*/true);
    REQUIRE(throwsError([&] { f16.est.SetSampleFormat(nrm, STATMC_SAMPLES_F32); }, STATMC_ERR_INVALID));   // afterwards: refused
    REQUIRE(throwsError([&] { f32.est.SetSampleFormat(nrm, STATMC_SAMPLES_F16); }, STATMC_ERR_INVALID));
    // the staging holds budget / bytes-per-pixel-sample pixel-samples per arena: 36 B in fp32, 12 + 6 + 6 = 24 B with the features half
    REQUIRE(EstimatorTestAccess::capacity(f32.est) == (int64_t)(budget / 36) / 4 * 4);
    REQUIRE(EstimatorTestAccess::capacity(f16.est) == (int64_t)(budget / 24) / 4 * 4);
    REQUIRE(f32.est.stagedBytes() == 0 && f16.est.stagedBytes() == 0);

    // one full 16 x 16 tile with 3 samples, then (after the flush) a clipped 13 x 8 tile with 2: the blocks start at element 0
    struct Case { Bounds2i b; int S; };
    const Case cases[2] = {{Bounds2i(Point2i(16, 16), Point2i(32, 32)), 3}, {Bounds2i(Point2i(32, 32), Point2i(45, 40)), 2}};
    size_t expect32 = 0, expect16 = 0;
    for (const Case &c : cases) {
        const int tw = c.b.pMax.x - c.b.pMin.x, th = c.b.pMax.y - c.b.pMin.y;
        for (Film *f : {&f32, &f16}) {
            auto lT = f->est.GetTiles<Vec3>(c.b, 1);
            auto fT = f->est.GetTiles<Vec3>(c.b, 1, 2);
            for (int s = 0; s < c.S; s++)
                for (int y = c.b.pMin.y; y < c.b.pMax.y; y++)
                    for (int x = c.b.pMin.x; x < c.b.pMax.x; x++) {
                        lT[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, s, 900.f));
                        fT[0][0].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 1.f));
                        fT[0][1].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 0.01f));
                    }
            f->est.MergeTransformTiles(lT, f->cfgs[Radiance]);
            f->est.MergeTiles(fT, std::vector<StatTypeConfig>{f->cfgs[StatNormal], f->cfgs[StatAlbedo]});
            f->est.Upload();   // dry run: the flush only counts
        }
        expect32 += (size_t)c.S * tw * th * 36;
        expect16 += (size_t)c.S * tw * th * 24;
        REQUIRE(f32.est.stagedBytes() == expect32);
        REQUIRE(f16.est.stagedBytes() == expect16);
        // block order [s][y][x][c]: radiance floats as recorded in both, the features as floats / as the converter's words
        const float *r32 = static_cast<const float *>(EstimatorTestAccess::staged(f32.est, rad, 0)), *r16 = static_cast<const float *>(EstimatorTestAccess::staged(f16.est, rad, 0));
        size_t e = 0;
        for (int s = 0; s < c.S; s++)
            for (int y = c.b.pMin.y; y < c.b.pMax.y; y++)
                for (int x = c.b.pMin.x; x < c.b.pMax.x; x++) {
                    const Vec3 L = sampleAt(x, y, s, 900.f), N = sampleAt(x, y, s, 1.f), A = sampleAt(x, y, s, 0.01f);
                    const float l[3] = {L.x, L.y, L.z}, n[3] = {N.x, N.y, N.z}, a[3] = {A.x, A.y, A.z};
                    for (int ch = 0; ch < 3; ch++, e++) {
                        REQUIRE(r32[e] == l[ch] && r16[e] == l[ch]);
                        REQUIRE(static_cast<const float *>(EstimatorTestAccess::staged(f32.est, nrm, 0))[e] == n[ch]);
                        REQUIRE(static_cast<const float *>(EstimatorTestAccess::staged(f32.est, alb, 0))[e] == a[ch]);
                        REQUIRE(static_cast<const uint16_t *>(EstimatorTestAccess::staged(f16.est, nrm, 0))[e] == floatToHalfBits(n[ch]));
                        REQUIRE(static_cast<const uint16_t *>(EstimatorTestAccess::staged(f16.est, alb, 0))[e] == floatToHalfBits(a[ch]));
                    }
                }
    }
    REQUIRE(f32.est.stagedMerges() == 6 && f16.est.stagedMerges() == 6 && f16.est.flushes() == 2);
    std::puts("tile half staging ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::string(argv[1]) == "convert") return convert(argv[2], argv[3]);
    if (argc == 2 && std::string(argv[1]) == "staging") return staging();
    std::fprintf(stderr, "usage: test_tile_half convert <in> <out> | staging\n");
    return 2;
}
