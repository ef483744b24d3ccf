// The chunk rule of statmc_accumulate_records_split and its argument check, from statmc_amd/csrc/statmc_records_plan.h compiled
// alone: no library, no device (tests/test_records_split_cpu.py compares the lines with a restatement of the rule, and builds
// this file once more with -fsanitize=address,undefined).
//   test_records_split_plan     prints, per count, "chunks <cnt> : begin len begin len ..." for the 64 slots, and per threshold
//                               "split_above <value> : ok" or the message that names the argument
#include <cstdint>
#include <cstdio>

#include "../../statmc_amd/csrc/statmc_records_plan.h"

int main() {
    static_assert(statmc::kRecSplitLanes == 64 && STATMC_RECORDS_SPLIT_LANES == 64, "a split pixel's slots are the lanes of one wave");
    static_assert(STATMC_RECORDS_SPLIT_DEFAULT >= 1, "the default threshold is a valid one");
    const int counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, (1 << 24) - 1, INT32_MAX};
    for (const int cnt : counts) {
        std::printf("chunks %d :", cnt);
        for (int slot = 0; slot < statmc::kRecSplitLanes; slot++) {
            int begin = -1, len = -1;
            statmc::records_split_chunk(cnt, slot, &begin, &len);
            std::printf(" %d %d", begin, len);
        }
        std::printf("\n");
    }
    const int32_t thresholds[] = {INT32_MIN, -1, 0, 1, 8, STATMC_RECORDS_SPLIT_DEFAULT, INT32_MAX};
    for (const int32_t v : thresholds) {
        char msg[128] = "";
        const bool ok = statmc::check_records_split_above(v, msg, sizeof(msg));
        std::printf("split_above %d : %s\n", (int)v, ok ? "ok" : msg);
    }
    return 0;
}
