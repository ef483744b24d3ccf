// CPU-only checks of ragged tiles in the Estimator's staging (include/statmc_denoiser.hpp), driven by
// tests/test_accumulate_counted_cpu.py: tiles whose pixels hold different sample counts merge, their slot is the bounding
// rectangle of the pixels with a count, S the largest count, the block is staged dense, and a flush with a ragged slot writes the
// per-pixel counts of all its slots into the film-sized count image.  A dry-run Estimator: links against libstatmc_hip.so only
// for the symbols; nothing here touches a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    struct SlotView {
        int x0, y0, x1, y1, samples;
        long long offset;
        std::vector<int32_t> counts;
    };
    static size_t slots(const Estimator &e) { return e.acc.slots.size(); }
    static SlotView slot(const Estimator &e, size_t k) {
        const auto &s = e.acc.slots.at(k);
        return SlotView{s.x0, s.y0, s.x1, s.y1, s.samples, (long long)s.offset, s.counts};
    }
    static const float *staged(const Estimator &e, unsigned char ti, unsigned char bj) { return e.acc.arenas.at(ti).at(bj).host.ptr; }
    // the film-sized count image the last counted flush wrote (NULL: no flush has staged counts)
    static const int32_t *counts(const Estimator &e) { return reinterpret_cast<const int32_t *>(e.acc.countsHost.ptr); }
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

static Vec3 sampleAt(int x, int y, int s, float scale) {
    const float v = scale * (1.0f + 0.001f * (float)(x + 37 * y) + 0.3331f * (float)s);
    return Vec3{v, v * 0.5f, v * 0.25f};
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

// the per-pixel budget of the test: 0 .. 5 samples, a column and a row of the tile without any
static int budget(int x, int y, const Bounds2i &b) {
    if (x == b.pMin.x || y == b.pMax.y - 1) return 0;
    return (x * 7 + y * 3) % 6;
}

int main() {
    const int W = 48, H = 40;
    Film f(W, H);
    f.est.EnableDeviceAccumulation((size_t)1 << 20, /*dryRun=*/true);
    const unsigned char rad = f.cfgs[Radiance].index;

    // ---- a flush of uniform tiles stages no counts
    const Bounds2i uni(Point2i(0, 0), Point2i(16, 16));
    {
        auto lT = f.est.GetTiles<Vec3>(uni, 1);
        auto fT = f.est.GetTiles<Vec3>(uni, 1, 2);
        for (int s = 0; s < 3; s++)
            for (int y = 0; y < 16; y++)
                for (int x = 0; x < 16; x++) {
                    lT[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, s, 9.f));
                    fT[0][0].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 1.f));
                    fT[0][1].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 0.01f));
                }
        f.est.MergeTransformTiles(lT, f.cfgs[Radiance]);
        f.est.MergeTiles(fT, std::vector<StatTypeConfig>{f.cfgs[StatNormal], f.cfgs[StatAlbedo]});
        REQUIRE(EstimatorTestAccess::slots(f.est) == 1 && EstimatorTestAccess::slot(f.est, 0).counts.empty());
        f.est.Upload();
    }
    REQUIRE(f.est.flushes() == 1 && f.est.countedFlushes() == 0);
    REQUIRE(EstimatorTestAccess::counts(f.est) == nullptr);
    size_t expectBytes = (size_t)3 * 16 * 16 * 36;
    REQUIRE(f.est.stagedBytes() == expectBytes);

    // ---- a ragged tile and a uniform one in one flush
    const Bounds2i rag(Point2i(16, 16), Point2i(32, 32)), uni2(Point2i(32, 16), Point2i(45, 32));
    {
        auto lT = f.est.GetTiles<Vec3>(rag, 1);
        auto fT = f.est.GetTiles<Vec3>(rag, 1, 2);
        int S = 0;
        for (int y = rag.pMin.y; y < rag.pMax.y; y++)
            for (int x = rag.pMin.x; x < rag.pMax.x; x++) {
                const int c = budget(x, y, rag);
                S = std::max(S, c);
                for (int s = 0; s < c; s++) {
                    lT[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, s, 9.f));
                    fT[0][0].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 1.f));
                    fT[0][1].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 0.01f));
                }
            }
        REQUIRE(S == 5);
        f.est.MergeTransformTiles(lT, f.cfgs[Radiance]);           // ragged tiles merge without throwing
        f.est.MergeTiles(fT, std::vector<StatTypeConfig>{f.cfgs[StatNormal], f.cfgs[StatAlbedo]});
        auto lU = f.est.GetTiles<Vec3>(uni2, 1);
        auto fU = f.est.GetTiles<Vec3>(uni2, 1, 2);
        for (int s = 0; s < 2; s++)
            for (int y = uni2.pMin.y; y < uni2.pMax.y; y++)
                for (int x = uni2.pMin.x; x < uni2.pMax.x; x++) {
                    lU[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, s, 9.f));
                    fU[0][0].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 1.f));
                    fU[0][1].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 0.01f));
                }
        f.est.MergeTransformTiles(lU, f.cfgs[Radiance]);
        f.est.MergeTiles(fU, std::vector<StatTypeConfig>{f.cfgs[StatNormal], f.cfgs[StatAlbedo]});

        // the slot: the bounding rectangle of the pixels with a count (the first column and the last row have none), S = 5
        REQUIRE(EstimatorTestAccess::slots(f.est) == 2);
        const auto s0 = EstimatorTestAccess::slot(f.est, 0), s1 = EstimatorTestAccess::slot(f.est, 1);
        REQUIRE(s0.x0 == 17 && s0.y0 == 16 && s0.x1 == 32 && s0.y1 == 31 && s0.samples == 5 && s0.offset == 0);
        REQUIRE(s0.counts.size() == (size_t)15 * 15);
        for (int y = 16; y < 31; y++)
            for (int x = 17; x < 32; x++) REQUIRE(s0.counts[(size_t)(y - 16) * 15 + (x - 17)] == budget(x, y, rag));
        REQUIRE(s1.x0 == 32 && s1.y0 == 16 && s1.x1 == 45 && s1.y1 == 32 && s1.samples == 2 && s1.counts.empty());
        REQUIRE(s1.offset == (5 * 15 * 15 + 3) / 4 * 4);
        // the block is staged dense, [s][y][x][c] over the rectangle: every live sample is where the tile entry reads it
        const float *r = EstimatorTestAccess::staged(f.est, rad, 0);
        for (int y = 16; y < 31; y++)
            for (int x = 17; x < 32; x++)
                for (int s = 0; s < budget(x, y, rag); s++) {
                    const Vec3 L = sampleAt(x, y, s, 9.f);
                    const size_t e = (((size_t)s * 15 + (y - 16)) * 15 + (x - 17)) * 3;
                    REQUIRE(r[e] == L.x && r[e + 1] == L.y && r[e + 2] == L.z);
                }
        f.est.Upload();
    }
    REQUIRE(f.est.flushes() == 2 && f.est.countedFlushes() == 1);
    // stagedBytes() keeps its formula: the sample bytes of the dense blocks
    expectBytes += ((size_t)5 * 15 * 15 + (size_t)2 * 13 * 16) * 36;
    REQUIRE(f.est.stagedBytes() == expectBytes);
    // the count image holds the counts of ALL slots of the flush: the ragged one's, and S for every pixel of the uniform one
    const int32_t *cnt = EstimatorTestAccess::counts(f.est);
    REQUIRE(cnt != nullptr);
    for (int y = 16; y < 31; y++)
        for (int x = 17; x < 32; x++) REQUIRE(cnt[(size_t)y * W + x] == budget(x, y, rag));
    for (int y = 16; y < 32; y++)
        for (int x = 32; x < 45; x++) REQUIRE(cnt[(size_t)y * W + x] == 2);

    // ---- the next flush of only uniform tiles stages no counts again
    {
        auto lT = f.est.GetTiles<Vec3>(uni, 1);
        for (int y = 0; y < 16; y++)
            for (int x = 0; x < 16; x++) lT[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, 0, 9.f));
        f.est.MergeTransformTiles(lT, f.cfgs[Radiance]);
        f.est.Upload();
    }
    REQUIRE(f.est.flushes() == 3 && f.est.countedFlushes() == 1);

    // ---- two stat types whose per-pixel counts disagree on one tile: still refused
    {
        auto lT = f.est.GetTiles<Vec3>(rag, 1);
        auto fT = f.est.GetTiles<Vec3>(rag, 1, 2);
        for (int y = rag.pMin.y; y < rag.pMax.y; y++)
            for (int x = rag.pMin.x; x < rag.pMax.x; x++) {
                const int c = 1 + (x + y) % 3;                      // the same rectangle and the same S for both ...
                for (int s = 0; s < c; s++) lT[0].AddTransformSampleM3(Point2i(x, y), sampleAt(x, y, s, 9.f));
                const int cf = (x == 20 && y == 20) ? (c % 3) + 1 : c;   // ... one pixel with another count
                for (int s = 0; s < cf; s++) fT[0][0].AddSampleM1(Point2i(x, y), sampleAt(x, y, s, 1.f));
            }
        f.est.MergeTransformTiles(lT, f.cfgs[Radiance]);
        REQUIRE(throwsError([&] { f.est.MergeTile(fT[0][0], f.cfgs[StatNormal].index, 0); }, STATMC_ERR_UNSUPPORTED));
    }
    std::puts("accumulate counted host ok");
    return 0;
}
