// statmc_compact_args.h on its own: no library, no device.  Every refusal of statmc_compact_offsets and statmc_compact_accumulate
// with the word its message must carry, the valid calls around them, the run clamp, the position-to-byte map above 2^31 and
// 2^33, and the workspace helper.  The image "pointers" are numbers: nothing is read through them.  Prints one line per failed
// expectation and "ok <n> checks"; exit status 0 when none failed.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_compact_args.h"

static int n_checks = 0, n_failed = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        n_checks++;                                                       \
        if (!(cond)) {                                                    \
            n_failed++;                                                   \
            printf("line %d: %s\n", __LINE__, #cond);                     \
        }                                                                 \
    } while (0)

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

static const uint64_t MIB = 1 << 20;
static const uint64_t COUNTS = 16 * MIB, OFFSETS = 32 * MIB, OWNERS = 48 * MIB, WS = 64 * MIB, ARENA = 80 * MIB, STATE = 96 * MIB;
static const int W = 64, H = 48;

struct OffsetsCall {
    int width = W, height = H;
    uint64_t counts = COUNTS, offsets = OFFSETS, owners = OWNERS, ws = WS;
    int32_t cap = INT32_MAX;
    int64_t capacity = 1000;
    int64_t ws_bytes = -1;   // -1: what the helper asks for
};
// "" for a valid call, else the message
static const char *offsets_verdict(const OffsetsCall &c) {
    static char why[512];
    why[0] = 0;
    const size_t need = statmc::compact_workspace_bytes((uint16_t)c.width, (uint16_t)c.height);
    const bool ok = statmc::check_compact_offsets_call((uint16_t)c.width, (uint16_t)c.height, at<int32_t>(c.counts), c.cap, at<int64_t>(c.offsets),
                                                       at<int32_t>(c.owners), c.capacity, at<void>(c.ws), c.ws_bytes < 0 ? need : (size_t)c.ws_bytes,
                                                       statmc::Msg{why, sizeof(why)});
    return ok ? "" : (why[0] ? why : "(refused without a message)");
}
static bool says(const char *verdict, const char *word) { return verdict[0] != 0 && strstr(verdict, word) != nullptr; }

static statmc_stat_type stat_type(uint64_t samples, int channels = 3) {
    statmc_stat_type t;
    memset(&t, 0, sizeof(t));
    t.channels = channels, t.transform = 1, t.max_moment = 3;
    t.samples = at<float>(samples);
    t.n = at<int32_t>(STATE);
    t.mean = at<float>(STATE + MIB), t.m2 = at<float>(STATE + 2 * MIB), t.m3 = at<float>(STATE + 3 * MIB);
    t.film_mean = at<float>(STATE + 4 * MIB), t.film_m2 = at<float>(STATE + 5 * MIB);
    return t;
}
static const char *accumulate_verdict(const statmc_stat_type *types, const int32_t *formats, int n_types, uint64_t offsets, int64_t n_samples,
                                      int32_t split_above) {
    static char why[512];
    why[0] = 0;
    const bool ok = statmc::check_compact_accumulate_call(types, formats, n_types, at<int64_t>(offsets), n_samples, split_above, statmc::Msg{why, sizeof(why)});
    return ok ? "" : (why[0] ? why : "(refused without a message)");
}

int main() {
    // ---- statmc_compact_offsets: every refusal, in the header's order, and the valid calls next to them
    {
        OffsetsCall c;
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.width = 0;
        EXPECT(says(offsets_verdict(c), "width"));
        c = OffsetsCall(), c.height = 0;
        EXPECT(says(offsets_verdict(c), "height"));
        c = OffsetsCall(), c.counts = 0;
        EXPECT(says(offsets_verdict(c), "null sample_counts"));
        c = OffsetsCall(), c.offsets = 0;
        EXPECT(says(offsets_verdict(c), "null offsets"));
        c = OffsetsCall(), c.ws = 0;
        EXPECT(says(offsets_verdict(c), "null workspace"));
        c = OffsetsCall(), c.counts += 2;
        EXPECT(says(offsets_verdict(c), "sample_counts is not 4-byte aligned"));
        c = OffsetsCall(), c.counts += 4;                      // a count image anywhere in a larger one
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.offsets += 4;
        EXPECT(says(offsets_verdict(c), "offsets is not 8-byte aligned"));
        c = OffsetsCall(), c.owners += 2;
        EXPECT(says(offsets_verdict(c), "owners is not 4-byte aligned"));
        c = OffsetsCall(), c.ws += 4;
        EXPECT(says(offsets_verdict(c), "workspace is not 8-byte aligned"));
        c = OffsetsCall(), c.cap = -1;
        EXPECT(says(offsets_verdict(c), "cap"));
        c = OffsetsCall(), c.cap = 0;
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.capacity = -1;
        EXPECT(says(offsets_verdict(c), "owners_capacity"));
        c = OffsetsCall(), c.owners = 0;
        EXPECT(says(offsets_verdict(c), "null owners"));
        c = OffsetsCall(), c.owners = 0, c.capacity = 0;
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.ws_bytes = (int64_t)statmc::compact_workspace_bytes(W, H) - 1;
        EXPECT(says(offsets_verdict(c), "workspace_bytes") && says(offsets_verdict(c), "24"));   // 3 blocks of 1024 pixels
        c = OffsetsCall(), c.ws_bytes = 4096;
        EXPECT(!offsets_verdict(c)[0]);
        const uint64_t px = (uint64_t)W * H;
        c = OffsetsCall(), c.offsets = COUNTS + px * 4 - 8;
        EXPECT(says(offsets_verdict(c), "offsets overlaps sample_counts"));
        c = OffsetsCall(), c.offsets = COUNTS + px * 4;        // right behind the counts
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.offsets = COUNTS - (px + 1) * 8;  // ends where the counts start
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.offsets = COUNTS - (px + 1) * 8 + 8;
        EXPECT(says(offsets_verdict(c), "offsets overlaps sample_counts"));
        c = OffsetsCall(), c.ws = OFFSETS + px * 8;            // over the total, offsets' last entry
        EXPECT(says(offsets_verdict(c), "offsets overlaps workspace"));
        c = OffsetsCall(), c.owners = COUNTS + 400;
        EXPECT(says(offsets_verdict(c), "owners overlaps sample_counts"));
        c = OffsetsCall(), c.owners = WS + 16;
        EXPECT(says(offsets_verdict(c), "owners overlaps workspace"));
        c = OffsetsCall(), c.owners = OFFSETS - 4000 + 4;      // 1000 slots: the last one over offsets[0]
        EXPECT(says(offsets_verdict(c), "owners overlaps offsets"));
        c = OffsetsCall(), c.owners = OFFSETS - 4000;
        EXPECT(!offsets_verdict(c)[0]);
        c = OffsetsCall(), c.owners = COUNTS, c.capacity = 0;  // no slots: owners is not looked at
        EXPECT(!offsets_verdict(c)[0]);

        statmc::CompactOffsetsArgs a;
        statmc::fill_compact_offsets_args(a, W, H, at<int32_t>(COUNTS), 7, at<int64_t>(OFFSETS), at<int32_t>(OWNERS), 1000, at<void>(WS));
        EXPECT(a.n_px == W * H && a.n_chunks == 3 && a.cap == 7 && a.vec == 1 && a.owners == at<int32_t>(OWNERS) && a.owners_capacity == 1000);
        statmc::fill_compact_offsets_args(a, 37, 29, at<int32_t>(COUNTS + 4), INT32_MAX, at<int64_t>(OFFSETS), at<int32_t>(OWNERS), 0, at<void>(WS));
        EXPECT(a.n_px == 37 * 29 && a.n_chunks == 2 && a.vec == 0 && a.owners == nullptr);
    }

    // ---- the workspace helper: 8-byte sized, monotone in the pixel count, one word per 1024 pixels
    {
        size_t before = 0;
        const int sizes[][2] = {{1, 1}, {3, 1}, {64, 16}, {1025, 1}, {37, 29}, {64, 48}, {1920, 1080}, {3840, 2160}, {65535, 65535}};
        for (const auto &s : sizes) {
            const size_t b = statmc::compact_workspace_bytes((uint16_t)s[0], (uint16_t)s[1]);
            const long long px = (long long)s[0] * s[1];
            EXPECT(b % 8 == 0 && b >= before && b == (size_t)((px + 1023) / 1024) * 8);
            before = b;
        }
        EXPECT(statmc::compact_workspace_bytes(1, 1) == 8 && statmc::compact_workspace_bytes(64, 16) == 8 && statmc::compact_workspace_bytes(1025, 1) == 16);
    }

    // ---- statmc_compact_accumulate: the refusals in the family's order
    {
        statmc_stat_type types[17];
        for (int i = 0; i < 17; i++) types[i] = stat_type(ARENA + (uint64_t)i * MIB, i % 2 ? 1 : 3);
        int32_t f32[16], f16[16], bad[16];
        for (int i = 0; i < 16; i++) f32[i] = STATMC_SAMPLES_F32, f16[i] = STATMC_SAMPLES_F16, bad[i] = i == 2 ? 7 : STATMC_SAMPLES_F32;
        EXPECT(!accumulate_verdict(types, nullptr, 4, OFFSETS, 1000, STATMC_RECORDS_SPLIT_DEFAULT)[0]);
        EXPECT(!accumulate_verdict(types, f32, 16, OFFSETS, 1000, INT32_MAX)[0]);
        EXPECT(!accumulate_verdict(types, f16, 16, OFFSETS, (int64_t)1 << 40, 1)[0]);
        EXPECT(says(accumulate_verdict(types, nullptr, 17, OFFSETS, 1000, 256), "n_types"));
        EXPECT(says(accumulate_verdict(types, nullptr, -1, OFFSETS, 1000, 256), "n_types"));
        EXPECT(says(accumulate_verdict(nullptr, nullptr, 4, OFFSETS, 1000, 256), "null types"));
        EXPECT(says(accumulate_verdict(types, nullptr, 4, 0, 1000, 256), "null offsets"));
        EXPECT(!accumulate_verdict(nullptr, nullptr, 0, 0, 1000, 256)[0]);      // zero types: a no-op
        EXPECT(!accumulate_verdict(nullptr, nullptr, 4, 0, 0, 256)[0]);         // zero samples: a no-op
        EXPECT(says(accumulate_verdict(types, nullptr, 4, OFFSETS, -1, 256), "n_samples"));
        EXPECT(says(accumulate_verdict(nullptr, nullptr, 4, 0, -1, 256), "null types"));   // the order: NULL with work to do first
        EXPECT(says(accumulate_verdict(types, bad, 4, OFFSETS, 1000, 256), "sample_formats[2]"));
        EXPECT(!accumulate_verdict(types, bad, 2, OFFSETS, 1000, 256)[0]);      // only the first n_types formats count
        types[1].samples = at<float>(ARENA + MIB + 1);
        EXPECT(says(accumulate_verdict(types, f16, 4, OFFSETS, 1000, 256), "types[1]") && says(accumulate_verdict(types, f16, 4, OFFSETS, 1000, 256), "odd"));
        types[1].samples = at<float>(ARENA + MIB + 2);
        EXPECT(!accumulate_verdict(types, f16, 4, OFFSETS, 1000, 256)[0]);      // a half arena at any even address
        EXPECT(says(accumulate_verdict(types, f32, 4, OFFSETS, 1000, 256), "types[1]") && says(accumulate_verdict(types, nullptr, 4, OFFSETS, 1000, 256), "4-byte"));
        types[1].samples = at<float>(ARENA + MIB + 4);
        EXPECT(!accumulate_verdict(types, nullptr, 4, OFFSETS, 1000, 256)[0]);  // an fp32 arena at any 4-byte boundary
        EXPECT(says(accumulate_verdict(types, nullptr, 4, OFFSETS + 4, 1000, 256), "offsets is not 8-byte aligned"));
        EXPECT(says(accumulate_verdict(types, nullptr, 4, OFFSETS, 1000, 0), "split_above"));
        EXPECT(says(accumulate_verdict(types, nullptr, 4, OFFSETS, 1000, -5), "split_above"));
        EXPECT(says(accumulate_verdict(types, nullptr, 4, OFFSETS + 4, 1000, 0), "offsets"));   // the order: alignment before split_above

        statmc::CompactArgs k;
        memset(&k, 0, sizeof(k));
        bool epilogue = true;
        char why[256] = "";
        types[0].transform = 5;
        EXPECT(statmc::fill_compact_args(k, W, H, types, f16, 4, at<int64_t>(OFFSETS), 1000, 32, epilogue, statmc::Msg{why, sizeof(why)}));
        EXPECT(k.n_types == 4 && k.n_px == W * H && k.n_samples == 1000 && k.half_mask == 15u && k.split_above == 32 && !epilogue);
        EXPECT(k.t[0].transform == 1 && k.t[1].channels == 1 && k.offsets == at<const long long>(OFFSETS));
        types[2].mean_corr = at<float>(STATE + 6 * MIB), types[2].discriminator = at<float>(STATE + 7 * MIB);
        EXPECT(statmc::fill_compact_args(k, W, H, types, nullptr, 4, at<int64_t>(OFFSETS), 1000, 32, epilogue, statmc::Msg{why, sizeof(why)}));
        EXPECT(epilogue && k.half_mask == 0u);
        types[3].channels = 2;
        EXPECT(!statmc::fill_compact_args(k, W, H, types, nullptr, 4, at<int64_t>(OFFSETS), 1000, 32, epilogue, statmc::Msg{why, sizeof(why)}));
        EXPECT(strstr(why, "types[3]") && strstr(why, "channels"));
    }

    // ---- the run clamp: whatever the offsets hold, 0 <= start <= end <= n_samples
    {
        const int64_t n = 1000, big = (int64_t)1 << 62;
        const int64_t pairs[][4] = {
            // o0, o1 -> start, end
            {10, 25, 10, 25},         {0, 0, 0, 0},           {990, 1000, 990, 1000},   {-5, 10, 0, 10},       {-5, -1, 0, 0},
            {30, 20, 30, 30},         {30, -7, 30, 30},       {990, 1010, 990, 1000},   {1000, 1001, 1000, 1000}, {1200, 1300, 1000, 1000},
            {1200, 5, 1000, 1000},    {-big, big, 0, 1000},   {big, -big, 1000, 1000},  {INT64_MIN, INT64_MAX, 0, 1000},
        };
        for (const auto &q : pairs) {
            int64_t s = -1, e = -1;
            statmc::compact_run(q[0], q[1], n, &s, &e);
            EXPECT(s == q[2] && e == q[3]);
            EXPECT(0 <= s && s <= e && e <= n);
        }
        int64_t s, e;
        statmc::compact_run(5, 9, 0, &s, &e);     // an arena of no samples: every run is empty
        EXPECT(s == 0 && e == 0);
        EXPECT(statmc::compact_run_count(10, 25) == 15 && statmc::compact_run_count(7, 7) == 0);
        EXPECT(statmc::compact_run_count(0, (int64_t)INT32_MAX) == INT32_MAX && statmc::compact_run_count(5, (int64_t)1 << 40) == INT32_MAX);
    }

    // ---- a position's byte offset in the arena: 64-bit, exact around and above 2^31 and 2^33
    {
        const int64_t positions[] = {0, 1, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 1, ((int64_t)1 << 32) + 5,
                                     ((int64_t)1 << 33) - 1, (int64_t)1 << 33, ((int64_t)1 << 33) + 12345, (int64_t)1 << 40};
        for (const int64_t at_pos : positions)
            for (const int channels : {1, 3})
                for (const bool half : {false, true})
                    for (const int64_t index : {(int64_t)0, (int64_t)1, (int64_t)299, ((int64_t)1 << 24) - 1}) {
                        const int64_t got = statmc::compact_sample_byte(at_pos, index, channels, half);
                        // the expectation in 128-bit arithmetic: nothing may wrap on the way
                        const __int128 want = ((__int128)at_pos + index) * channels * (half ? 2 : 4);
                        EXPECT((__int128)got == want);
                        EXPECT(got >= 0 && got % (half ? 2 : 4) == 0);
                    }
        EXPECT(statmc::compact_sample_byte((int64_t)1 << 31, 0, 3, false) == (int64_t)25769803776);   // 2^31 * 12: beyond 32 bits twice over
        EXPECT(statmc::compact_sample_byte((int64_t)1 << 33, 1, 1, true) == (int64_t)17179869186);
        // consecutive samples lie channels * element bytes apart, also across 2^31
        EXPECT(statmc::compact_sample_byte(((int64_t)1 << 31) - 1, 1, 3, false) - statmc::compact_sample_byte(((int64_t)1 << 31) - 1, 0, 3, false) == 12);
        EXPECT(statmc::compact_sample_byte(((int64_t)1 << 31) - 1, 1, 3, true) - statmc::compact_sample_byte(((int64_t)1 << 31) - 1, 0, 3, true) == 6);
    }

    printf("%s %d checks", n_failed ? "FAILED" : "ok", n_checks);
    if (n_failed) printf(", %d failed", n_failed);
    printf("\n");
    return n_failed ? 1 : 0;
}
