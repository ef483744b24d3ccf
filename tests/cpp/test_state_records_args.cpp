// statmc_state_records_args.h on its own: no library, no device.  The dwords of a state record for every kind of stat type and
// for values no type can have, every refusal of statmc_gather_states and statmc_combine_records with the word its message must
// carry, the valid calls and the no-ops around them, and what the argument block holds.  The device "pointers" are numbers:
// nothing is read through them.  Prints one line per failed expectation and "ok <n> checks"; exit status 0 when none failed.
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_state_records_args.h"

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
static const uint64_t PIXELS = 16 * MIB, RECORDS = 32 * MIB, STATE = 96 * MIB;
static const int W = 64, H = 48;

static statmc_stat_type stat_type(int channels = 3, int transform = 1, int max_moment = 3) {
    statmc_stat_type t;
    memset(&t, 0, sizeof(t));
    t.channels = channels, t.transform = transform, t.max_moment = max_moment;
    t.n = at<int32_t>(STATE);
    t.mean = at<float>(STATE + MIB), t.m2 = at<float>(STATE + 2 * MIB), t.m3 = at<float>(STATE + 3 * MIB);
    t.film_mean = at<float>(STATE + 4 * MIB), t.film_m2 = at<float>(STATE + 5 * MIB);
    return t;
}

struct Call {
    int width = W, height = H, n_types = 4;
    bool types = true, states = true;
    uint64_t pixels = PIXELS;
    int64_t n_records = 1000;
    int32_t split_above = STATMC_RECORDS_SPLIT_DEFAULT;
    uint64_t record_arrays[17];
    statmc_stat_type t[17];
    Call() {
        for (int i = 0; i < 17; i++) {
            record_arrays[i] = RECORDS + (uint64_t)i * MIB;
            t[i] = stat_type(i % 2 ? 1 : 3, i % 3 == 0, 1 + i % 3);
        }
    }
};
// "" for a valid call, else the message; combine: statmc_combine_records' check, else statmc_gather_states'
static const char *verdict(const Call &c, bool combine) {
    static char why[512];
    why[0] = 0;
    const void *states[17];
    for (int i = 0; i < 17; i++) states[i] = at<void>(c.record_arrays[i]);
    const statmc::Msg m{why, sizeof(why)};
    const bool ok = combine ? statmc::check_combine_records_call((uint16_t)c.width, (uint16_t)c.height, c.types ? c.t : nullptr, c.n_types,
                                                                 at<int32_t>(c.pixels), c.n_records, c.states ? states : nullptr, c.split_above, m)
                            : statmc::check_gather_states_call((uint16_t)c.width, (uint16_t)c.height, c.types ? c.t : nullptr, c.n_types,
                                                               at<int32_t>(c.pixels), c.n_records, c.states ? states : nullptr, m);
    return ok ? "" : (why[0] ? why : "(refused without a message)");
}
static bool says(const char *v, const char *word) { return v[0] != 0 && strstr(v, word) != nullptr; }

int main() {
    // ---- the dwords of a record: 1 + C (M + 2 T) for the twelve kinds, 0 for everything else
    for (int c = -1; c <= 5; c++)
        for (int m = -1; m <= 5; m++)
            for (int t = 0; t <= 2; t++) {
                const bool kind = (c == 1 || c == 3) && m >= 1 && m <= 3;
                EXPECT(statmc::state_record_dwords(c, m, t) == (kind ? (size_t)(1 + c * (m + (t ? 2 : 0))) : (size_t)0));
            }
    EXPECT(statmc::state_record_dwords(3, 3, 1) == 16 && statmc::state_record_dwords(3, 1, 0) == 4 && statmc::state_record_dwords(1, 1, 0) == 2);
    EXPECT(statmc::state_record_dwords(3, 3, 7) == 16 && statmc::state_record_dwords(3, 3, -1) == 16);      // transform: zero or not
    EXPECT(statmc::state_record_dwords(2, 3, 1) == 0 && statmc::state_record_dwords(3, 0, 1) == 0 && statmc::state_record_dwords(3, 4, 0) == 0);

    // ---- both entries: every refusal, in the header's order, and the valid calls next to them
    for (const bool combine : {false, true}) {
        Call c;
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.n_types = 16;
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.n_types = 17;
        EXPECT(says(verdict(c, combine), "n_types"));
        c = Call(), c.n_types = -1;
        EXPECT(says(verdict(c, combine), "n_types"));
        c = Call(), c.n_records = -1;
        EXPECT(says(verdict(c, combine), "n_records"));
        c = Call(), c.n_records = (int64_t)1 << 31;
        EXPECT(says(verdict(c, combine), "n_records"));
        c = Call(), c.n_records = ((int64_t)1 << 31) - 1;
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.n_types = 17, c.n_records = -1;                // the order: the type limit first
        EXPECT(says(verdict(c, combine), "n_types"));
        c = Call(), c.types = false;
        EXPECT(says(verdict(c, combine), "null types"));
        c = Call(), c.pixels = 0;
        EXPECT(says(verdict(c, combine), "null pixels"));
        c = Call(), c.states = false;
        EXPECT(says(verdict(c, combine), "null states"));
        c = Call(), c.pixels += 2;
        EXPECT(says(verdict(c, combine), "pixels is not 4-byte aligned"));
        c = Call(), c.pixels += 4;                                   // a list anywhere in a larger one
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.record_arrays[2] = 0;
        EXPECT(says(verdict(c, combine), "states[2] is null"));
        c = Call(), c.record_arrays[3] += 2;
        EXPECT(says(verdict(c, combine), "states[3] is not 4-byte aligned"));
        c = Call(), c.record_arrays[3] += 4;
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.record_arrays[4] = 0;                          // only the first n_types arrays count
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.width = 0;
        EXPECT(says(verdict(c, combine), "width"));
        c = Call(), c.height = 0;
        EXPECT(says(verdict(c, combine), "height"));
        // zero types or zero records: a no-op whatever the pointers and the film hold
        c = Call(), c.n_types = 0, c.types = false, c.states = false, c.pixels = 0, c.width = 0;
        EXPECT(!verdict(c, combine)[0]);
        c = Call(), c.n_records = 0, c.types = false, c.states = false, c.pixels = 2, c.height = 0;
        EXPECT(!verdict(c, combine)[0]);
    }
    // ---- split_above: the combine's alone, behind the limits and ahead of the pointers
    {
        Call c;
        c.split_above = 1;
        EXPECT(!verdict(c, true)[0]);
        c.split_above = INT32_MAX;
        EXPECT(!verdict(c, true)[0]);
        c.split_above = 0;
        EXPECT(says(verdict(c, true), "split_above") && !verdict(c, false)[0]);
        c.split_above = -5;
        EXPECT(says(verdict(c, true), "split_above"));
        c.n_records = 0;                                             // refused ahead of the no-op
        EXPECT(says(verdict(c, true), "split_above"));
        c.n_records = -1;
        EXPECT(says(verdict(c, true), "n_records"));
        c = Call(), c.split_above = 0, c.types = false;
        EXPECT(says(verdict(c, true), "split_above"));
    }

    // ---- the argument block
    {
        Call c;
        const void *states[17];
        for (int i = 0; i < 17; i++) states[i] = at<void>(c.record_arrays[i]);
        statmc::StateRecordsArgs k;
        memset(&k, 0, sizeof(k));
        bool epilogue = true;
        char why[256] = "";
        const statmc::Msg m{why, sizeof(why)};
        c.t[0].transform = 5;
        c.t[0].n_samples = 77;
        EXPECT(statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        EXPECT(k.n_types == 4 && k.n_px == W * H && k.n_records == 1000 && k.split_above == 32 && !epilogue && k.pixels == at<int32_t>(PIXELS));
        EXPECT(k.t[0].transform == 1 && k.t[0].n_samples == 0 && k.t[1].channels == 1 && k.t[2].samples == at<float>(RECORDS + 2 * MIB));
        for (int i = 0; i < 4; i++) EXPECT(k.dwords[i] == (int)statmc::state_record_dwords(c.t[i].channels, c.t[i].max_moment, c.t[i].transform));
        EXPECT(k.dwords[0] == 10 && k.dwords[1] == 3 && k.dwords[2] == 10 && k.dwords[3] == 4);
        // the epilogue: the combine's, max_moment 3; the gather ignores the two pointers
        c.t[2].mean_corr = at<float>(STATE + 6 * MIB), c.t[2].discriminator = at<float>(STATE + 7 * MIB);
        EXPECT(statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        EXPECT(epilogue && k.t[2].mean_corr == at<float>(STATE + 6 * MIB));
        EXPECT(statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, INT32_MAX, true, epilogue, m));
        EXPECT(!epilogue && k.t[2].mean_corr == nullptr && k.t[2].discriminator == nullptr);
        c.t[1].mean_corr = at<float>(STATE + 6 * MIB), c.t[1].discriminator = at<float>(STATE + 7 * MIB);     // max_moment 2
        EXPECT(!statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        EXPECT(strstr(why, "types[1]") && strstr(why, "max_moment 3"));
        EXPECT(statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, true, epilogue, m));
        c = Call();
        c.t[3].channels = 2;
        EXPECT(!statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, true, epilogue, m));
        EXPECT(strstr(why, "types[3]") && strstr(why, "channels"));
        c = Call();
        c.t[0].m3 = nullptr;                                         // types[0]: 3 channels, transform, max_moment 1 -- m3 is not needed
        EXPECT(statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        c.t[2].m3 = nullptr;                                         // types[2]: max_moment 3
        EXPECT(!statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        EXPECT(strstr(why, "types[2]") && strstr(why, "m3"));
        c = Call();
        c.t[0].film_mean = nullptr;
        EXPECT(!statmc::fill_state_records_args(k, W, H, c.t, 4, at<int32_t>(PIXELS), 1000, states, 32, false, epilogue, m));
        EXPECT(strstr(why, "types[0]") && strstr(why, "film_mean"));
    }

    printf("%s %d checks", n_failed ? "FAILED" : "ok", n_checks);
    if (n_failed) printf(", %d failed", n_failed);
    printf("\n");
    return n_failed ? 1 : 0;
}
