// statmc_accumulate_args.h without a device and without the library: every check and fill the accumulation entries share, over a
// fixed case list.  One line per case, which tests/test_accumulate_args_cpu.py compares with tests/golden/accumulate_args.json:
//   <group> <name> : ok [what was filled] | <the message>
// The pointers are made up; nothing is read through them.  Planes are printed as byte offsets from their made-up base.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../statmc_amd/csrc/statmc_accumulate_args.h"

using namespace statmc;

namespace {

char g_msg[256];
const Msg M{g_msg, sizeof(g_msg)};
const int kTable = 4, kFlags = 3;    // a pre-pass table and flags that no default could be mistaken for

// plane j of type i: a made-up 16-byte aligned address, 1 GiB from the next
uintptr_t base(int i, int j) { return 0x100000000000ull + ((uintptr_t)i << 36) + ((uintptr_t)j << 30); }
template <class T> T *at(int i, int j) { return reinterpret_cast<T *>(base(i, j)); }
enum { SAMPLES, N, MEAN, M2, M3, FILM_MEAN, FILM_M2, MEAN_CORR, DISC, COUNTS };

// a valid type: every plane its max_moment and transform ask for, the epilogue pair if asked for
statmc_stat_type type(int i, int channels, int transform, int max_moment, int n_samples = 2, bool epilogue = false) {
    statmc_stat_type t{};
    t.channels = channels, t.transform = transform, t.max_moment = max_moment, t.n_samples = n_samples;
    t.samples = at<const float>(i, SAMPLES), t.n = at<int32_t>(i, N), t.mean = at<float>(i, MEAN);
    if (max_moment >= 2) t.m2 = at<float>(i, M2);
    if (max_moment >= 3) t.m3 = at<float>(i, M3);
    if (transform) t.film_mean = at<float>(i, FILM_MEAN), t.film_m2 = at<float>(i, FILM_M2);
    if (epilogue) t.mean_corr = at<float>(i, MEAN_CORR), t.discriminator = at<float>(i, DISC);
    return t;
}
long long off(const void *p, int i, int j) { return p ? (long long)(reinterpret_cast<uintptr_t>(p) - base(i, j)) : -1; }

void verdict(const char *group, const std::string &name, bool ok, const std::string &filled = "") {
    std::printf("%s %s : %s%s\n", group, name.c_str(), ok ? "ok" : g_msg, ok ? filled.c_str() : "");
}
std::string str(const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0, long long f = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c, d, e, f);
    return buf;
}
// what fill_stat_type wrote, the planes of entry `d` (type i) as byte offsets (-1: NULL)
std::string entry(const AccumulateType &d, int i) {
    return str(" ch%lld s%lld tr%lld mm%lld pre%lld/%lld", d.channels, d.n_samples, d.transform, d.max_moment, d.pre_table, d.pre_flags) +
           str(" elems%lld stride%lld |", d.n_elems, d.stride) + str(" %lld %lld %lld %lld", off(d.samples, i, SAMPLES), off(d.n, i, N), off(d.mean, i, MEAN), off(d.m2, i, M2)) +
           str(" %lld %lld %lld %lld %lld", off(d.m3, i, M3), off(d.film_mean, i, FILM_MEAN), off(d.film_m2, i, FILM_M2), off(d.mean_corr, i, MEAN_CORR), off(d.disc, i, DISC));
}

void oneType(const std::string &name, statmc_stat_type t, bool batch = true) {
    AccumulateType d{};
    const bool ok = fill_stat_type(kTable, kFlags, t, 7, 12, 5, batch, d, M);
    verdict("type", name + str(" c%lld", t.channels), ok, ok ? entry(d, 0) : "");
}

ArenaCall arena(uint16_t w, uint16_t h, const std::vector<statmc_stat_type> &types, const int32_t *formats, const int32_t *counts) {
    return ArenaCall{w, h, types.empty() ? nullptr : types.data(), (int)types.size(), formats, counts, nullptr};
}
// fill_row_range_entries into the uncounted or, with counts, the counted block: every entry on a line of its own
void film(const std::string &name, const std::vector<statmc_stat_type> &types, const std::vector<int32_t> &formats, const std::vector<int32_t> &ranges,
          bool counted = false, bool details = true) {
    const int32_t *counts = counted ? at<const int32_t>(0, COUNTS) : nullptr;
    const FilmCall c{arena(12, 5, types, formats.empty() ? nullptr : formats.data(), counts), ranges.data(), (int)ranges.size() / 2, false};
    AccumulateArgs k{};
    AccumulateCountedArgs kc{};
    const bool ok = counted ? fill_row_range_entries(kc, kTable, kFlags, c, kc.counts, M) : fill_row_range_entries(k, kTable, kFlags, c, nullptr, M);
    const int n = counted ? kc.n_types : k.n_types, mask = counted ? kc.half_mask : k.half_mask;
    verdict("film", name, ok, str(" entries%lld half_mask0x%llx", n, mask));
    for (int e = 0; ok && details && e < n; e++) {
        const AccumulateType &d = counted ? kc.t[e] : k.t[e];
        int i = 0;   // the type the entry came from: its n plane lies in that type's made-up block
        while (reinterpret_cast<uintptr_t>(d.n) < base(i, N) || reinterpret_cast<uintptr_t>(d.n) >= base(i, N + 1)) i++;
        std::printf("film %s entry %d : type%d%s%s\n", name.c_str(), e, i, entry(d, i).c_str(),
                    counted ? str(" counts%lld", off(kc.counts[e], 0, COUNTS)).c_str() : "");
    }
}

}  // namespace

int main() {
    // ---- one descriptor: each refusal for 1- and 3-channel types, and what a valid one becomes
    for (int ch : {1, 3}) {
        oneType("mean only", type(0, ch, 0, 1));
        oneType("three moments, transform", type(0, ch, 1, 3));
        oneType("epilogue", type(0, ch, 1, 3, 2, true));
        oneType("tile-fed: n_samples ignored", type(0, ch, 0, 2, -5), false);
        oneType("max_moment 0", type(0, ch, 0, 0));
        oneType("max_moment 4", type(0, ch, 0, 4));
        statmc_stat_type t = type(0, ch, 0, 2);
        t.m2 = nullptr;
        oneType("no m2", t);
        t = type(0, ch, 0, 3);
        t.m3 = nullptr;
        oneType("no m3", t);
        t = type(0, ch, 1, 1);
        t.film_mean = nullptr;
        oneType("transform without film_mean", t);
        t = type(0, ch, 1, 1);
        t.film_m2 = nullptr;
        oneType("transform without film_m2", t);
        t = type(0, ch, 0, 3, 2, true);
        t.discriminator = nullptr;
        oneType("mean_corr alone", t);
        t = type(0, ch, 0, 3, 2, true);
        t.mean_corr = nullptr;
        oneType("discriminator alone", t);
        oneType("epilogue with max_moment 2", type(0, ch, 0, 2, 2, true));
        oneType("negative n_samples", type(0, ch, 0, 1, -1));
        t = type(0, ch, 0, 1, 0);
        t.samples = nullptr;
        oneType("no samples, n_samples 0", t);
        oneType("no samples, tile-fed", t, false);
        t = type(0, ch, 0, 1);
        t.n = nullptr;
        oneType("no n", t);
    }
    oneType("channels", type(0, 2, 0, 1));

    // ---- the type-count limit
    for (int n : {-1, 0, 16, 17}) verdict("limit", str("n_types %lld", n), check_type_limit(n, nullptr, M));
    const int limits[][2] = {{2, 9}, {2, 8}, {16, 1}, {17, 1}, {17, 0}, {0, 1000}, {-1, 1}, {1, -1}, {65536, 65536}};
    for (const auto &l : limits) verdict("limit", str("n_types %lld x n_ranges %lld", l[0], l[1]), check_type_limit(l[0], &l[1], M));
    for (int n : {-1, 0, 1}) verdict("limit", str("n_tiles %lld", n), check_n_tiles(n, M));

    // ---- the row ranges of a 12 x 5 film: the default, the bounds, the overlap rule, the pointer advance, the half mask
    const std::vector<statmc_stat_type> rgb3 = {type(0, 3, 1, 3, 2, true)}, two = {type(0, 3, 1, 3), type(1, 1, 0, 1)};
    const int32_t some[4] = {0, 1, 2, 3};
    struct { const char *name; const int32_t *ranges; int n; } defaults[] = {{"NULL, 0", nullptr, 0}, {"ranges, 0", some, 0}, {"NULL, 2", nullptr, 2},
                                                                               {"NULL, -1", nullptr, -1}, {"ranges, 2", some, 2}};
    for (const auto &d : defaults) {
        FilmCall c{arena(12, 5, two, nullptr, nullptr), d.ranges, d.n, true};
        int32_t whole[2] = {-7, -7};
        const bool ok = default_row_ranges(c, whole, M);
        verdict("ranges default", d.name, ok, ok ? str(" n_ranges%lld [%lld,%lld) ", c.n_ranges, c.ranges[0], c.ranges[1]) + (c.ranges == whole ? "whole" : "given") : "");
    }
    film("rows [0,6)", two, {}, {0, 6}, false, false);
    film("rows [-1,2)", two, {}, {-1, 2}, false, false);
    film("rows [3,2) reversed", two, {}, {3, 2}, false, false);
    film("rows [0,3) [2,5) overlap", two, {}, {0, 3, 2, 5}, false, false);
    film("rows [2,5) [0,3) overlap", two, {}, {2, 5, 0, 3}, false, false);
    film("rows [0,2) [2,5) touch", two, {}, {0, 2, 2, 5}, false, false);
    film("rows [2,2) empty", two, {}, {2, 2});
    film("rows [0,1) [3,3) [4,5), one empty", two, {}, {0, 1, 3, 3, 4, 5}, false, false);
    film("rows [5,5) empty at the end", two, {}, {5, 5}, false, false);
    film("an invalid type behind an empty range", {type(0, 2, 0, 1)}, {}, {2, 2}, false, false);
    film("types[1] invalid", {type(0, 3, 0, 1), type(1, 3, 0, 0)}, {}, {0, 5}, false, false);
    film("advance f32 rows [3,5)", rgb3, {STATMC_SAMPLES_F32}, {3, 5});
    film("advance half rows [3,5)", rgb3, {STATMC_SAMPLES_F16}, {3, 5});
    film("advance 1-channel half rows [3,4)", {type(0, 1, 0, 1)}, {STATMC_SAMPLES_F16}, {3, 4});
    film("advance counted rows [3,5)", rgb3, {}, {3, 5}, true);
    const std::vector<statmc_stat_type> three = {type(0, 3, 1, 3), type(1, 3, 0, 1), type(2, 1, 0, 1)};
    film("half mask, 2 ranges x (f32, half, half)", three, {0, 1, 1}, {0, 2, 3, 5});
    film("half mask, 3 ranges x (half, f32, half), one empty", three, {1, 0, 1}, {0, 1, 2, 2, 4, 5}, false, false);
    std::vector<statmc_stat_type> wide(2, type(0, 1, 0, 1));
    film("2 types x 8 ranges", wide, {}, {0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5}, false, false);

    // ---- the counted entry leaves entries with n_samples == 0 out; the uncounted entry keeps them
    const std::vector<statmc_stat_type> middle0 = {type(0, 3, 1, 3), type(1, 3, 0, 1, 0), type(2, 1, 0, 1)};
    film("counted, middle n_samples 0, last half", middle0, {0, 0, 1}, {0, 5}, true);
    film("counted, the same over 2 ranges", middle0, {0, 0, 1}, {0, 2, 3, 5}, true);
    film("uncounted, the same", middle0, {0, 0, 1}, {0, 5});
    film("counted, every n_samples 0", {type(0, 3, 0, 1, 0), type(1, 1, 0, 1, 0)}, {1, 1}, {0, 5}, true);
    std::vector<statmc_stat_type> bad_middle = middle0;
    bad_middle[1].mean = nullptr;
    film("counted, middle n_samples 0 without mean", bad_middle, {}, {0, 5}, true);

    // ---- sample formats, odd arenas, counts, and what runs ahead of the device
    const int32_t *aligned = at<const int32_t>(0, COUNTS);
    std::vector<statmc_stat_type> odd = two;
    odd[1].samples = reinterpret_cast<const float *>(base(1, SAMPLES) + 1);
    const int32_t f32s[17] = {}, halfs[2] = {0, 1}, bad_first[2] = {2, 0}, bad_last[2] = {1, -1};
    verdict("formats", "NULL", check_sample_formats(nullptr, 2, M));
    verdict("formats", "(f32, half)", check_sample_formats(halfs, 2, M), str(" half_mask0x%llx", half_mask_of(halfs, 2)));
    verdict("formats", "bad first", check_sample_formats(bad_first, 2, M));
    verdict("formats", "bad last", check_sample_formats(bad_last, 2, M));
    verdict("arenas", "odd half arena", check_sample_arenas(arena(12, 5, odd, halfs, nullptr), M));
    verdict("arenas", "odd fp32 arena (the kernels' scalar path)", check_sample_arenas(arena(12, 5, odd, f32s, nullptr), M));
    verdict("arenas", "odd arena, no formats", check_sample_arenas(arena(12, 5, odd, nullptr, aligned), M));
    for (int k = 1; k <= 3; k++)
        verdict("arenas", str("counts + %lld", k), check_sample_arenas(arena(12, 5, two, nullptr, reinterpret_cast<const int32_t *>(base(0, COUNTS) + k)), M));
    verdict("arenas", "counts + 4", check_sample_arenas(arena(12, 5, two, halfs, aligned + 1), M));
    verdict("arenas", "counts + 1 before a bad format", check_sample_arenas(arena(12, 5, two, bad_first, reinterpret_cast<const int32_t *>(base(0, COUNTS) + 1)), M));
    verdict("arenas", "a bad format before null types", check_sample_arenas(ArenaCall{12, 5, nullptr, 2, bad_last, aligned, nullptr}, M));
    verdict("arenas", "null types", check_sample_arenas(ArenaCall{12, 5, nullptr, 2, halfs, nullptr, nullptr}, M));
    verdict("arenas", "null types, n_types 0", check_sample_arenas(ArenaCall{12, 5, nullptr, 0, nullptr, aligned, nullptr}, M));
    const std::vector<statmc_stat_type> seventeen(17, type(0, 3, 0, 1));
    const int one = 1, minus = -1, nine = 9;
    struct { const char *name; ArenaCall c; const int *n_ranges, *n_tiles; } ahead[] = {
        {"neither formats nor counts: 17 types pass", arena(12, 5, seventeen, nullptr, nullptr), &one, nullptr},
        {"neither: n_tiles -1 passes", arena(12, 5, two, nullptr, nullptr), nullptr, &minus},
        {"formats: 17 types", arena(12, 5, seventeen, f32s, nullptr), &one, nullptr},
        {"formats: 2 types x 9 ranges", arena(12, 5, two, f32s, nullptr), &nine, nullptr},
        {"formats all f32: null types pass", ArenaCall{12, 5, nullptr, 2, f32s, nullptr, nullptr}, &one, nullptr},
        {"formats with a half: null types", ArenaCall{12, 5, nullptr, 2, halfs, nullptr, nullptr}, &one, nullptr},
        {"formats with a half: n_tiles -1 passes", arena(12, 5, two, halfs, nullptr), nullptr, &minus},
        {"formats with a half: odd arena", arena(12, 5, odd, halfs, nullptr), nullptr, &one},
        {"formats: the limit before a bad format", arena(12, 5, seventeen, bad_first, nullptr), nullptr, &one},
        {"counts: null types", ArenaCall{12, 5, nullptr, 2, nullptr, aligned, nullptr}, &one, nullptr},
        {"counts: n_types 0 passes", ArenaCall{12, 5, nullptr, 0, nullptr, aligned, nullptr}, &one, nullptr},
        {"counts: n_tiles -1", arena(12, 5, two, nullptr, aligned), nullptr, &minus},
        {"counts: n_types before n_tiles", arena(12, 5, seventeen, nullptr, aligned), nullptr, &minus},
        {"counts: n_tiles before the alignment", arena(12, 5, two, nullptr, reinterpret_cast<const int32_t *>(base(0, COUNTS) + 2)), nullptr, &minus},
        {"counts: 2 types x 9 ranges", arena(12, 5, two, nullptr, aligned), &nine, nullptr},
        {"counts and halves: valid", arena(12, 5, two, halfs, aligned), &one, nullptr},
    };
    for (const auto &a : ahead) verdict("ahead", a.name, check_ahead_of_device(a.c, a.n_ranges, a.n_tiles, M));

    // ---- the tile descriptors, in either argument block
    const int32_t tile_formats[3] = {0, 1, 0};
    const TilesCall tc{arena(12, 5, three, tile_formats, aligned), at<const int32_t>(3, 0), at<const int64_t>(3, 1), at<const int32_t>(3, 2), 6};
    AccumulateTilesArgs tk{};
    AccumulateTilesCountedArgs tkc{};
    TilesCall tc2 = tc;
    tc2.n_types = 2;    // (the third type and format are not looked at)
    for (int counted = 0; counted < 2; counted++) {
        const bool ok = counted ? fill_tiles_args(tkc, kTable, kFlags, tc2, M) : fill_tiles_args(tk, kTable, kFlags, tc2, M);
        const long long fields[6] = {counted ? tkc.n_types : tk.n_types, counted ? tkc.half_mask : tk.half_mask, counted ? tkc.n_tiles : tk.n_tiles,
                                     counted ? tkc.width : tk.width, counted ? tkc.height : tk.height, 0};
        verdict("tiles", counted ? "counted block" : "uncounted block", ok,
                str(" types%lld half_mask0x%llx tiles%lld %lldx%lld", fields[0], fields[1], fields[2], fields[3], fields[4]) +
                    str(" | %lld %lld %lld", off(counted ? tkc.tile_bounds : tk.tile_bounds, 3, 0), off(counted ? tkc.tile_offsets : tk.tile_offsets, 3, 1),
                        off(counted ? tkc.tile_samples : tk.tile_samples, 3, 2)) + " |" + entry(counted ? tkc.t[1] : tk.t[1], 1));
    }
    TilesCall tc3 = tc;
    const std::vector<statmc_stat_type> tile_bad = {type(0, 3, 0, 1), type(1, 3, 1, 3, -1, true), type(2, 1, 0, 4)};
    tc3.types = tile_bad.data();
    verdict("tiles", "types[2] invalid, negative n_samples ignored", fill_tiles_args(tk, kTable, kFlags, tc3, M));

    // ---- the records entries' types
    const std::vector<statmc_stat_type> rec = {type(0, 3, 7, 3, -3, true), type(1, 1, 0, 1)};
    for (int interleaved = 0; interleaved < 2; interleaved++) {
        std::vector<statmc_stat_type> types = rec;
        if (interleaved) types[1].samples = nullptr;    // an interleaved call's descriptors need no samples
        const RecordsCall rc{12, 5, types.data(), 2, at<const int32_t>(3, 0), interleaved ? at<const void>(3, 1) : nullptr, nullptr, interleaved != 0, 100, nullptr, nullptr};
        RecordsArgs rk{};
        RecordsInterleavedArgs rik{};
        bool epilogue = false;
        const bool ok = interleaved ? fill_records_args(rik, rc, epilogue, M) : fill_records_args(rk, rc, epilogue, M);
        const statmc_stat_type *t = interleaved ? rik.t : rk.t;
        verdict("records", interleaved ? "interleaved" : "record-major", ok,
                str(" types%lld records%lld px%lld epilogue%lld", interleaved ? rik.n_types : rk.n_types, interleaved ? rik.n_records : rk.n_records,
                    interleaved ? rik.n_px : rk.n_px, epilogue) +
                    str(" | tr%lld s%lld samples %lld %lld mean_corr %lld", t[0].transform, t[0].n_samples, off(t[0].samples, 0, SAMPLES), off(t[1].samples, 1, SAMPLES),
                        off(t[0].mean_corr, 0, MEAN_CORR)));
        if (!interleaved) {
            types[1].samples = nullptr;
            verdict("records", "record-major without samples", fill_records_args(rk, rc, epilogue, M));
        }
        types[1].samples = rec[1].samples;
        types[1].mean_corr = at<float>(1, MEAN_CORR);
        verdict("records", interleaved ? "interleaved, types[1] half an epilogue" : "record-major, types[1] half an epilogue", fill_records_args(rk, rc, epilogue, M));
    }
    return 0;
}
