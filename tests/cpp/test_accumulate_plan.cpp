// statmc::plan_accumulate over a fixed list of launches: films on either side of every group-count threshold, every batch-length
// threshold, the type sets the fused walk takes and refuses, every mix of sample formats, misaligned arenas, row ranges and each
// debug knob on its own, and last every (K, M) x format instantiation of the fused walk.  Nothing is launched and no device is
// looked at: the pointers are made up (and aligned as a caller's would be).  One line per case, which
// tests/test_accumulate_plan_cpu.py compares with tests/golden/accumulate_plan.json:
//   name : grid fused loader kernel vec dma umul grid_mode resident_blocks K M fmt lds
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../statmc_amd/csrc/statmc_device.h"

using namespace statmc;

namespace {

struct Kind { int channels, transform, max_moment; };
const Kind RAD{3, 1, 3}, RGB{3, 0, 1}, F1{1, 0, 1};
struct TypeSet { const char *name; std::vector<Kind> kinds; };
const TypeSet kSets[] = {
    {"rad", {RAD}},                         // radiance alone
    {"five", {RAD, RGB, RGB, F1, F1}},      // the 11-channel five
    {"three", {RAD, RGB, RGB}},             // the 9-channel three
    {"rad+f1", {RAD, F1}},
    {"rad2", {RAD, RAD}},                   // two radiance types: not fusable
    {"rad+rgb3", {RAD, RGB, RGB, RGB}},     // K > 2: not fusable
};
const TypeSet &kFive = kSets[1];
// every (K, M) the fused walk is instantiated for: K mean-only RGB types, M mean-only 1-channel types beside the radiance type
// (a list of its own: the loops over kSets keep their cases)
const TypeSet kFusedSets[] = {
    {"k0m1", {RAD, F1}},          {"k0m2", {RAD, F1, F1}},      {"k1m0", {RAD, RGB}},          {"k1m1", {RAD, RGB, F1}},
    {"k1m2", {RAD, RGB, F1, F1}}, {"k2m0", {RAD, RGB, RGB}},    {"k2m1", {RAD, RGB, RGB, F1}}, {"k2m2", {RAD, RGB, RGB, F1, F1}},
};
enum { F32 = 0, FEAT16, ALL16, RAD16 };
const char *kFmtName[] = {"f32", "feat16", "all16", "rad16"};

struct Knobs { int resident_blocks = 0, umul = 1, dma = 1, grid_mode = -1, fused = 0; };
struct Film { int w, h; };

// The argument statmc_accumulate_formats builds for rows [y0, y1) of a w x h film (statmc_abi.hip), every plane of every type a
// made-up address 1 MiB-aligned; sample_shift[i] bytes are added to type i's arena.
AccumulateArgs makeArgs(Film film, int y0, int y1, int n_samples, const TypeSet &set, int fmt, int apart, int cus, const Knobs &k,
                        const std::vector<int> &sample_shift = {}, int n_ranges = 1) {
    AccumulateArgs a{};
    for (int r = 0; r < n_ranges; r++) {
        const int r0 = r == 0 ? y0 : film.h - (y1 - y0), r1 = r == 0 ? y1 : film.h;     // a second range: the film's last rows
        for (size_t i = 0; i < set.kinds.size(); i++) {
            const Kind &kind = set.kinds[i];
            AccumulateType &t = a.t[a.n_types];
            const bool half = fmt == ALL16 || (fmt == FEAT16 && i > 0) || (fmt == RAD16 && i == 0);
            const uintptr_t base = 0x700000000000ull + ((uintptr_t)i << 40);
            const uintptr_t e0 = (uintptr_t)r0 * film.w * kind.channels;
            const uintptr_t shift = i < sample_shift.size() ? sample_shift[i] : 0;
            auto plane = [&](int j) { return reinterpret_cast<float *>(base + ((uintptr_t)j << 36) + 4 * e0); };
            t.samples = reinterpret_cast<const float *>(base + (half ? 2 : 4) * e0 + shift);
            t.n = reinterpret_cast<int32_t *>(base + ((uintptr_t)1 << 36) + 4 * (uintptr_t)r0 * film.w);
            t.mean = plane(2);
            if (kind.max_moment >= 2) t.m2 = plane(3);
            if (kind.max_moment >= 3) t.m3 = plane(4);
            if (kind.transform) { t.film_mean = plane(5); t.film_m2 = plane(6); }
            if (kind.max_moment >= 3) { t.mean_corr = plane(7); t.disc = plane(8); }       // the radiance type's pre-pass epilogue
            t.n_elems = (long long)(r1 - r0) * film.w * kind.channels;
            t.stride = (long long)film.h * film.w * kind.channels;
            t.channels = kind.channels;
            t.n_samples = n_samples;
            t.transform = kind.transform;
            t.max_moment = kind.max_moment;
            if (half) a.half_mask |= 1 << a.n_types;
            a.n_types++;
        }
    }
    a.resident_blocks = k.resident_blocks;
    a.cus = cus;
    a.umul = k.umul;
    a.dma = k.dma;
    a.grid_mode = k.grid_mode;
    a.fused = k.fused;
    a.apart = apart;
    return a;
}

void show(const std::string &name, const AccumulateArgs &a) {
    static std::set<std::string> seen;      // the sweeps below overlap: every case once
    if (!seen.insert(name).second) return;
    const AccumulatePlan p = plan_accumulate(a, nullptr);
    std::printf("%s : %u %d %d %d %d %d %d %d %d %d %d %d %zu\n", name.c_str(), p.grid, p.kernel == kAccFused || p.kernel == kAccFusedHalf,
                p.loader, p.kernel, p.vec, p.dma, p.umul, p.grid_mode, p.resident_blocks, p.K, p.M, p.fmt, p.lds);
}

std::string nameOf(Film f, int s, const TypeSet &set, int fmt, int apart, int cus) {
    char buf[128];
    std::snprintf(buf, sizeof(buf), "%dx%d s%d %s %s", f.w, f.h, s, set.name, kFmtName[fmt]);
    return std::string(buf) + (apart ? "" : " apart0") + (cus == 256 ? "" : " cus" + std::to_string(cus));
}
void whole(Film f, int s, const TypeSet &set, int fmt, int apart, int cus) {
    show(nameOf(f, s, set, fmt, apart, cus), makeArgs(f, 0, f.h, s, set, fmt, apart, cus, Knobs{}));
}

}  // namespace

int main() {
    // (62 x 8 is 124 whole groups; 62 x 9 ends in half a group)
    const Film named[] = {{64, 8}, {62, 8}, {62, 9}, {256, 4}, {960, 540}, {1280, 720}, {1600, 900}, {1920, 1080}, {2048, 1152}, {2560, 1440}, {3840, 2160}};
    // one film below and one at each group-count threshold (a group is 4 pixels): 128 000, 2^18, 2^19, 3 x 2^18, 2^20; and one on
    // either side of "the last of 8 walks of 256 workgroups is 97 % full" (508 560 groups)
    const Film edges[] = {{1000, 511}, {1000, 512}, {1024, 1023}, {1024, 1024}, {2048, 1023}, {2048, 1024}, {2048, 1535}, {2048, 1536},
                          {2048, 2047}, {2048, 2048}, {1920, 1059}, {1920, 1060}};
    const int batches[] = {1, 4, 8, 9, 16, 17, 64, 127, 128, 255, 256};
    const Film hd{1920, 1080}, uhd{3840, 2160};
    std::vector<Film> films(named, named + 11);
    films.insert(films.end(), edges, edges + 12);

    // every film x every batch length: the five types, fp32, placed buffers
    for (const Film &f : films)
        for (int s : batches) whole(f, s, kFive, F32, 1, 256);
    // ... torch's allocator (apart = 0): the rule reads the batch length at 8 and 16 and the film at 2^20 groups
    for (const Film &f : films)
        for (int s : {8, 9, 16, 17, 128, 256})
            if ((f.w != 1000 && f.w != 1920) || f.h == 1080) whole(f, s, kFive, F32, 0, 256);
    // ... the feature types half: no rule reads the batch length (the threshold films at one length only)
    for (const Film &f : films)
        for (int s : {1, 16, 256})
            if (s == 256 || &f < &films[11]) whole(f, s, kFive, FEAT16, 1, 256);
    // every type set x every mix of formats (a lone radiance type has no feature types: feat16 is f32 there)
    for (const TypeSet &set : kSets)
        for (int fmt : {F32, FEAT16, ALL16, RAD16})
            for (const Film &f : {Film{64, 8}, Film{62, 9}, hd, uhd})
                for (int s : {16, 256})
                    if (!(fmt == FEAT16 && set.kinds.size() == 1)) whole(f, s, set, fmt, 1, 256);
    // a device whose CU count is not known (cus = 0)
    for (const Film &f : named)
        for (int s : {16, 128, 256}) whole(f, s, kFive, F32, 1, 0);
    for (const Film &f : {hd, uhd})
        for (int s : {16, 128, 256}) {
            whole(f, s, kFive, F32, 0, 0);
            whole(f, s, kFive, FEAT16, 1, 0);
        }
    // row ranges of a 1080p film (n_elems < stride): its first 20 rows, and its first and last 20 rows in one launch
    for (int fmt : {F32, FEAT16, ALL16})
        for (int s : {16, 256})
            for (int n_ranges : {1, 2})
                show(nameOf(hd, s, kFive, fmt, 1, 256) + " rows20x" + std::to_string(n_ranges), makeArgs(hd, 0, 20, s, kFive, fmt, 1, 256, Knobs{}, {}, n_ranges));
    // misaligned arenas: an fp32 one at + 4 bytes, a half one at + 2 and + 8; a half film of a multiple of 4 but not of 8 pixels
    for (const Film &f : {Film{64, 8}, hd})
        for (int s : {16, 256}) {
            show(nameOf(f, s, kFive, F32, 1, 256) + " rad+4B", makeArgs(f, 0, f.h, s, kFive, F32, 1, 256, Knobs{}, {4}));
            show(nameOf(f, s, kFive, F32, 1, 256) + " f1+4B", makeArgs(f, 0, f.h, s, kFive, F32, 1, 256, Knobs{}, {0, 0, 0, 4}));
            show(nameOf(f, s, kFive, FEAT16, 1, 256) + " rad+4B", makeArgs(f, 0, f.h, s, kFive, FEAT16, 1, 256, Knobs{}, {4}));
            for (int fmt : {FEAT16, ALL16})
                for (int shift : {2, 8})
                    show(nameOf(f, s, kFive, fmt, 1, 256) + " rgb+" + std::to_string(shift) + "B", makeArgs(f, 0, f.h, s, kFive, fmt, 1, 256, Knobs{}, {0, shift}));
        }
    for (const Film &f : {Film{60, 9}, Film{1924, 1079}})
        for (int fmt : {F32, FEAT16, ALL16, RAD16}) whole(f, 256, kFive, fmt, 1, 256);
    // each debug knob on its own (and the deeper prefetch where it shows: without the LDS-DMA ring)
    struct Named { const char *name; Knobs k; };
    std::vector<Named> knobs;
    auto knob = [&](const char *name, auto set) { Knobs k; set(k); knobs.push_back({name, k}); };
    knob("resident-1", [](Knobs &k) { k.resident_blocks = -1; });
    knob("resident64", [](Knobs &k) { k.resident_blocks = 64; });
    knob("fused-1", [](Knobs &k) { k.fused = -1; });
    knob("fused1", [](Knobs &k) { k.fused = 1; });
    knob("dma0", [](Knobs &k) { k.dma = 0; });
    knob("grid_mode0", [](Knobs &k) { k.grid_mode = 0; });
    knob("grid_mode1", [](Knobs &k) { k.grid_mode = 1; });
    knob("umul2", [](Knobs &k) { k.umul = 2; });
    knob("dma0+umul2", [](Knobs &k) { k.dma = 0; k.umul = 2; });
    for (const Named &kn : knobs)
        for (int s : {256, 16})
            for (int fmt : {F32, FEAT16})
                show(nameOf(hd, s, kFive, fmt, 1, 256) + " " + kn.name, makeArgs(hd, 0, hd.h, s, kFive, fmt, 1, 256, kn.k));
    // every instantiation of the fused walk, asked for on one workgroup's film (tests/test_accumulate_fused_sets_gpu.py runs them)
    Knobs fused1;
    fused1.fused = 1;
    for (const TypeSet &set : kFusedSets)
        for (int fmt : {F32, FEAT16, ALL16})
            show(nameOf(Film{256, 4}, 4, set, fmt, 1, 256) + " fused1", makeArgs(Film{256, 4}, 0, 4, 4, set, fmt, 1, 256, fused1));
    return 0;
}
