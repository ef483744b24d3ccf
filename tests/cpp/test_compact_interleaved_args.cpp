// statmc_compact_interleaved_args.h on its own: no library, no device.  Every refusal of statmc_compact_accumulate_interleaved in
// the documented order with the word its message must carry, the valid calls around them, the run clamp on record positions, the
// position-to-byte map above 2^31 and 2^33 at strides 28, 44, 48 and 52, the argument fill and the plan's type sets.  The image
// "pointers" are numbers: nothing is read through them.  Prints one line per failed expectation and "ok <n> checks"; exit status
// 0 when none failed.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_compact_interleaved_args.h"

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
static const uint64_t OFFSETS = 32 * MIB, RECORDS = 80 * MIB, STATE = 96 * MIB;
static const int W = 64, H = 48;

static statmc_stat_type stat_type(int channels, int transform, int max_moment) {
    statmc_stat_type t;
    memset(&t, 0, sizeof(t));
    t.channels = channels, t.transform = transform, t.max_moment = max_moment;
    t.n = at<int32_t>(STATE);
    t.mean = at<float>(STATE + MIB), t.m2 = at<float>(STATE + 2 * MIB), t.m3 = at<float>(STATE + 3 * MIB);
    t.film_mean = at<float>(STATE + 4 * MIB), t.film_m2 = at<float>(STATE + 5 * MIB);
    return t;
}

// the shipped 11-channel set in a 44-byte record: radiance, albedo, normal, depth, id
struct Call {
    statmc_stat_type types[17];
    statmc_record_layout layout;
    int n_types = 5;
    bool has_types = true, has_layout = true;
    uint64_t records = RECORDS, offsets = OFFSETS;
    int64_t n_records = 1000;
    int32_t split_above = 256;
    Call() {
        memset(&layout, 0, sizeof(layout));
        for (int i = 0; i < 17; i++) types[i] = stat_type(1, 0, 1);
        types[0] = stat_type(3, 1, 3);
        types[1] = stat_type(3, 0, 1);
        types[2] = stat_type(3, 0, 1);
        layout.stride = 44;
        layout.pixel_offset = -12345;   // garbage: never read
        const int off[5] = {0, 12, 24, 36, 40};
        for (int i = 0; i < 5; i++) layout.sample_offset[i] = off[i];
    }
};
static char why[512];
// "" for a valid call, else the message
static const char *verdict(const Call &c) {
    why[0] = 0;
    const bool ok = statmc::check_compact_interleaved_call(c.has_types ? c.types : nullptr, c.n_types, at<void>(c.records), c.has_layout ? &c.layout : nullptr,
                                                           at<int64_t>(c.offsets), c.n_records, c.split_above, statmc::Msg{why, sizeof(why)});
    return ok ? "" : (why[0] ? why : "(refused without a message)");
}
static bool says(const char *v, const char *word) { return v[0] != 0 && strstr(v, word) != nullptr; }

int main() {
    // ---- valid calls
    {
        Call c;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.split_above = INT32_MAX;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.n_records = (int64_t)1 << 33;                     // no 2^31 limit
        EXPECT(!verdict(c)[0]);
        c = Call(), c.n_records = (int64_t)INT32_MAX + 1;
        EXPECT(!verdict(c)[0]);
        for (int px : {INT32_MIN, -4, -1, 0, 2, 41, 44, 1 << 30, INT32_MAX}) {   // pixel_offset: neither read nor checked
            c = Call(), c.layout.pixel_offset = px;
            EXPECT(!verdict(c)[0]);
        }
        c = Call(), c.records += 4;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.layout.stride = 48;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.layout.stride = 4, c.n_types = 1, c.types[0] = stat_type(1, 0, 1);
        EXPECT(!verdict(c)[0]);
        c = Call();                                                       // fields in reverse order, overlapping, half
        const int off[5] = {32, 20, 20, 4, 0};
        for (int i = 0; i < 5; i++) c.layout.sample_offset[i] = off[i];
        EXPECT(!verdict(c)[0]);
        c = Call(), c.layout.sample_format[3] = STATMC_SAMPLES_F16, c.layout.sample_offset[3] = 38;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.n_types = 16, c.layout.stride = 64;
        for (int i = 5; i < 16; i++) c.layout.sample_offset[i] = 4 * i;
        EXPECT(!verdict(c)[0]);
        // zero types or zero records: a no-op, whatever the pointers
        c = Call(), c.n_types = 0, c.has_types = false, c.has_layout = false, c.records = 0, c.offsets = 0;
        EXPECT(!verdict(c)[0]);
        c = Call(), c.n_records = 0, c.has_types = false, c.has_layout = false, c.records = 0, c.offsets = 0;
        EXPECT(!verdict(c)[0]);
    }
    // ---- every refusal, and the documented order: an earlier rule wins over every later one
    {
        Call c;
        c.n_types = 17;
        EXPECT(says(verdict(c), "n_types"));
        c = Call(), c.n_types = -1;
        EXPECT(says(verdict(c), "n_types"));
        c = Call(), c.has_types = false;
        EXPECT(says(verdict(c), "null types"));
        c = Call(), c.has_layout = false;
        EXPECT(says(verdict(c), "null layout"));
        c = Call(), c.records = 0;
        EXPECT(says(verdict(c), "null records"));
        c = Call(), c.offsets = 0;
        EXPECT(says(verdict(c), "null offsets"));
        c = Call(), c.n_records = -1;
        EXPECT(says(verdict(c), "n_records"));
        for (int stride : {0, 2, -4, 46, 3}) {
            c = Call(), c.layout.stride = stride;
            EXPECT(says(verdict(c), "stride"));
        }
        for (int d : {1, 2, 3}) {
            c = Call(), c.records += d;
            EXPECT(says(verdict(c), "records must be 4-byte aligned"));
        }
        c = Call(), c.layout.sample_format[2] = 7;
        EXPECT(says(verdict(c), "sample_format[2]"));
        c = Call(), c.types[1].channels = 2;
        EXPECT(says(verdict(c), "types[1].channels"));
        c = Call(), c.types[4].channels = 0;
        EXPECT(says(verdict(c), "types[4].channels"));
        c = Call(), c.layout.sample_offset[0] = -4;
        EXPECT(says(verdict(c), "sample_offset[0]"));
        c = Call(), c.layout.sample_offset[1] = 14;                      // fp32 at a 2-byte boundary
        EXPECT(says(verdict(c), "sample_offset[1]"));
        c = Call(), c.layout.sample_offset[2] = 36;                      // 12 bytes from 36 end at 48 > 44
        EXPECT(says(verdict(c), "sample_offset[2]"));
        c = Call(), c.layout.sample_offset[4] = 44;
        EXPECT(says(verdict(c), "sample_offset[4]"));
        c = Call(), c.layout.sample_format[3] = STATMC_SAMPLES_F16, c.layout.sample_offset[3] = 37;   // half at an odd offset
        EXPECT(says(verdict(c), "sample_offset[3]"));
        for (int d : {1, 2, 4}) {
            c = Call(), c.offsets += d;
            EXPECT(says(verdict(c), "offsets is not 8-byte aligned"));
        }
        for (int s : {0, -1, INT32_MIN}) {
            c = Call(), c.split_above = s;
            EXPECT(says(verdict(c), "split_above"));
        }
        // the order: each call breaks rule k and every rule behind it; rule k is the one named
        const char *order[] = {"n_types", "null types", "null layout", "null records", "null offsets", "n_records", "stride", "records must be",
                               "sample_format[0]", "types[0].channels", "sample_offset[0]", "offsets is not", "split_above"};
        const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
        for (int k = 0; k < n_rules; k++) {
            c = Call();
            // (a NULL pointer is not also misaligned, a NULL layout has no fields: those later rules cannot be broken together
            // with the NULL, every other one is)
            if (k <= 0) c.n_types = 17;
            if (k <= 1) c.has_types = false;
            if (k <= 2) c.has_layout = false;
            if (k <= 3) c.records = 0;
            if (k <= 4) c.offsets = 0;
            if (k <= 5) c.n_records = -5;
            if (k <= 6) c.layout.stride = 6;
            if (k <= 7 && k > 3) c.records += 2;
            if (k <= 8) c.layout.sample_format[0] = 9;
            if (k <= 9) c.types[0].channels = 4;
            if (k <= 10) c.layout.sample_offset[0] = 42;
            if (k <= 11 && k > 4) c.offsets += 4;
            if (k <= 12) c.split_above = 0;
            EXPECT(says(verdict(c), order[k]));
        }
        // without work NULL pointers are no refusal, the rest still is
        c = Call(), c.n_records = 0, c.records = 0, c.offsets = 0, c.split_above = 0;
        EXPECT(says(verdict(c), "split_above"));
        c = Call(), c.n_types = 0, c.layout.stride = 6;
        EXPECT(says(verdict(c), "stride"));
    }
    // ---- the clamp (compact_run, unchanged) on record positions, and the 32-bit run count
    {
        const int64_t n = ((int64_t)1 << 33) + 7;
        const int64_t cases[][4] = {{0, 4, 0, 4},      {4, 4, 4, 4},       {-3, 9, 0, 9},        {9, 7, 9, 9},       {7, n + 50, 7, n},
                                    {n + 1, n + 9, n, n}, {-9, -2, 0, 0},  {INT64_MIN, INT64_MAX, 0, n}, {INT64_MAX, INT64_MIN, n, n}, {n - 1, n, n - 1, n}};
        for (const auto &q : cases) {
            int64_t s = -1, e = -1;
            statmc::compact_run(q[0], q[1], n, &s, &e);
            EXPECT(s == q[2] && e == q[3]);
            EXPECT(0 <= s && s <= e && e <= n);
        }
        EXPECT(statmc::compact_run_count(0, n) == INT32_MAX);
        EXPECT(statmc::compact_run_count(5, 305) == 300);
        EXPECT(statmc::compact_run_count(n, n) == 0);
    }
    // ---- compact_record_byte: 64-bit, above 2^31 and 2^33 records
    {
        const int64_t positions[] = {0, 1, 65535, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 12345, (int64_t)1 << 33,
                                     ((int64_t)1 << 33) + 987654321, ((int64_t)1 << 40) + 3};
        for (int stride : {28, 44, 48, 52})
            for (int64_t pos : positions)
                for (int off : {0, 4, 22, stride - 4}) {
                    const int64_t b = statmc::compact_record_byte(pos, stride, off);
                    // the expectation without a 64-bit product: stride = 4 q + ..., summed in pieces that cannot wrap
                    int64_t want = off;
                    for (int k = 0; k < stride; k += 4) want += 4 * pos;
                    EXPECT(b == want);
                    EXPECT(b >= pos && (b - off) % stride == 0 && (b - off) / stride == pos);
                }
        EXPECT(statmc::compact_record_byte((int64_t)1 << 31, 44, 40) == 94489280552ll);
        EXPECT(statmc::compact_record_byte(((int64_t)1 << 33) + 1, 52, 0) == 446676598836ll);
    }
    // ---- the fill, and the plan's type sets
    {
        Call c;
        c.layout.sample_format[3] = STATMC_SAMPLES_F16;
        statmc::CompactInterleavedArgs k;
        memset(&k, 0, sizeof(k));
        bool epilogue = true;
        why[0] = 0;
        EXPECT(statmc::fill_compact_interleaved_args(k, W, H, c.types, 5, at<void>(RECORDS), c.layout, at<int64_t>(OFFSETS), (int64_t)1 << 33, 300, epilogue,
                                                     statmc::Msg{why, sizeof(why)}));
        EXPECT(!epilogue && k.n_types == 5 && k.n_px == W * H && k.n_records == (int64_t)1 << 33 && k.split_above == 300 && k.stride == 44);
        EXPECT(k.half_mask == 8u && k.off[0] == 0 && k.off[1] == 12 && k.off[2] == 24 && k.off[3] == 36 && k.off[4] == 40);
        EXPECT(k.records == at<char>(RECORDS) && k.offsets == at<long long>(OFFSETS));
        for (int i = 0; i < 5; i++) EXPECT(k.t[i].samples == nullptr && k.t[i].n == c.types[i].n && k.t[i].transform == (i == 0));
        c.types[0].mean_corr = at<float>(STATE + 6 * MIB), c.types[0].discriminator = at<float>(STATE + 7 * MIB);
        EXPECT(statmc::fill_compact_interleaved_args(k, W, H, c.types, 5, at<void>(RECORDS), c.layout, at<int64_t>(OFFSETS), 10, 300, epilogue,
                                                     statmc::Msg{why, sizeof(why)}) && epilogue);
        c.types[2].max_moment = 4;                                       // the descriptors' own rules
        EXPECT(!statmc::fill_compact_interleaved_args(k, W, H, c.types, 5, at<void>(RECORDS), c.layout, at<int64_t>(OFFSETS), 10, 300, epilogue,
                                                      statmc::Msg{why, sizeof(why)}) && strstr(why, "types[2]"));
        c.types[2].max_moment = 1, c.types[1].mean = nullptr;
        EXPECT(!statmc::fill_compact_interleaved_args(k, W, H, c.types, 5, at<void>(RECORDS), c.layout, at<int64_t>(OFFSETS), 10, 300, epilogue,
                                                      statmc::Msg{why, sizeof(why)}) && strstr(why, "types[1]"));
    }
    {
        using namespace statmc;
        Call c;
        int kernel = -1;
        RecordsInterleavedPlan p = plan_compact_interleaved(c.types, 5, c.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel == kCompactIlvDefault && (kernel == kCompactIlvFusedStaged || kernel == kCompactIlvFusedDirect));
        EXPECT(p.path == kRecIlvFused && p.K == 2 && p.M == 2 && p.fmt == 0);
        EXPECT(p.order[0] == 0 && p.order[1] == 1 && p.order[2] == 2 && p.order[3] == 3 && p.order[4] == 4);
        for (int force : {kCompactIlvFusedStaged, kCompactIlvFusedDirect}) {
            plan_compact_interleaved(c.types, 5, c.layout, force, &kernel);
            EXPECT(kernel == force);
        }
        p = plan_compact_interleaved(c.types, 5, c.layout, kCompactIlvGeneral, &kernel);
        EXPECT(kernel == kCompactIlvGeneral && p.path == kRecIlvGeneral);
        // every K, M of the fused fold, in any order of the types
        for (int K = 0; K <= 2; K++)
            for (int M = 0; M <= 2; M++) {
                statmc_stat_type t[5];
                int n = 0;
                for (int i = 0; i < M; i++) t[n++] = stat_type(1, 0, 1);
                const int rad = n;
                t[n++] = stat_type(3, 1, 3);
                for (int i = 0; i < K; i++) t[n++] = stat_type(3, 0, 1);
                p = plan_compact_interleaved(t, n, c.layout, kCompactIlvFusedStaged, &kernel);
                if (K + M == 0) {
                    EXPECT(kernel == kCompactIlvGeneral);
                    continue;
                }
                EXPECT(kernel == kCompactIlvFusedStaged && p.K == K && p.M == M && p.order[0] == rad);
                for (int i = 0; i < K; i++) EXPECT(p.order[1 + i] == rad + 1 + i);
                for (int i = 0; i < M; i++) EXPECT(p.order[1 + K + i] == i);
            }
        // the format classes: 0 all fp32, 1 the features half, 2 the radiance too; anything mixed is the general kernel's
        Call h;
        for (int i = 1; i < 5; i++) h.layout.sample_format[i] = STATMC_SAMPLES_F16;
        p = plan_compact_interleaved(h.types, 5, h.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel != kCompactIlvGeneral && p.fmt == 1);
        h.layout.sample_format[0] = STATMC_SAMPLES_F16;
        p = plan_compact_interleaved(h.types, 5, h.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel != kCompactIlvGeneral && p.fmt == 2);
        h.layout.sample_format[2] = STATMC_SAMPLES_F32;
        plan_compact_interleaved(h.types, 5, h.layout, kCompactIlvFusedStaged, &kernel);
        EXPECT(kernel == kCompactIlvGeneral);
        h = Call(), h.layout.sample_format[0] = STATMC_SAMPLES_F16;     // a half radiance with fp32 features
        plan_compact_interleaved(h.types, 5, h.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel == kCompactIlvGeneral);
        // type sets outside the fused fold
        Call g;
        g.types[1] = stat_type(3, 0, 2);                                 // a second moment on a feature
        plan_compact_interleaved(g.types, 5, g.layout, kCompactIlvFusedDirect, &kernel);
        EXPECT(kernel == kCompactIlvGeneral);
        g = Call(), g.types[1] = stat_type(3, 1, 3);                     // two radiance types
        plan_compact_interleaved(g.types, 5, g.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel == kCompactIlvGeneral);
        g = Call(), g.types[3] = stat_type(3, 0, 1);                     // three mean-only RGB types
        plan_compact_interleaved(g.types, 5, g.layout, kCompactIlvAuto, &kernel);
        EXPECT(kernel == kCompactIlvGeneral);
        g = Call();
        plan_compact_interleaved(g.types, 1, g.layout, kCompactIlvAuto, &kernel);    // one type
        EXPECT(kernel == kCompactIlvGeneral);
        g.n_types = 6;
        plan_compact_interleaved(g.types, 6, g.layout, kCompactIlvAuto, &kernel);    // six
        EXPECT(kernel == kCompactIlvGeneral);
        EXPECT(compact_interleaved_window_valid(kCompactIlvWindowDefault) && compact_interleaved_window_valid(1024) && compact_interleaved_window_valid(65536));
        EXPECT(!compact_interleaved_window_valid(0) && !compact_interleaved_window_valid(1536) && !compact_interleaved_window_valid(66560));
    }
    if (n_failed) {
        printf("%d of %d checks failed\n", n_failed, n_checks);
        return 1;
    }
    printf("ok %d checks\n", n_checks);
    return 0;
}
