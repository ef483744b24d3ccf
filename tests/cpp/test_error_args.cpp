// statmc_error_args.h on its own: no library, no device, nothing but include/statmc.h (and statmc_plan_args.h, which it builds on).
// Reads a table of calls -- the one tests/test_error_scores_cpu.py writes from its restatement of include/statmc.h -- and prints
// check_error_scores_call's / check_target_call's verdict for each, and for the valid ones what fill_error_args / fill_target_args
// made of them.  The image "pointers" of the table are numbers: nothing is read through them.
//
//   error <name> <width> <height> <channels> <metric> <eps as float bits> <table>  <n film_mean film_m2 score>
//   target <name> <width> <height> <target as float bits> <c_min> <c_max>  <error n sample_counts result>
//
// Output, one line per call:   <name> : ok error <vec> <has table>   |   <name> : ok target <chunks> <grid> <vec>   |   <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_error_args.h"

static_assert(sizeof(statmc_target_result) == 48, "statmc_target_result is 48 bytes");

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <table>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        int width, height;
        why[0] = 0;
        if (strcmp(word, "error") == 0) {
            int channels, metric, table;
            uint32_t eps_bits;
            uint64_t p[4];
            if (fscanf(f, "%127s %d %d %d %d %" SCNu32 " %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, name, &width, &height, &channels, &metric,
                       &eps_bits, &table, &p[0], &p[1], &p[2], &p[3]) != 11) {
                fprintf(stderr, "bad error line\n");
                return 2;
            }
            float eps;
            memcpy(&eps, &eps_bits, sizeof(eps));
            if (!statmc::check_error_scores_call((uint16_t)width, (uint16_t)height, channels, metric, eps, table, at<int32_t>(p[0]), at<float>(p[1]),
                                                 at<float>(p[2]), at<float>(p[3]), statmc::PlanMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                static const float some_table[1] = {0.f};   // stands for the device's table: never read
                statmc::ErrorArgs a;
                statmc::fill_error_args(a, (uint16_t)width, (uint16_t)height, channels, metric, eps, table >= 0 ? some_table : nullptr, at<int32_t>(p[0]),
                                        at<float>(p[1]), at<float>(p[2]), at<float>(p[3]));
                printf("%s : ok error %d %d\n", name, a.vec, a.tq != nullptr);
            }
        } else if (strcmp(word, "target") == 0) {
            uint32_t target_bits;
            int c_min, c_max;
            uint64_t p[4];
            if (fscanf(f, "%127s %d %d %" SCNu32 " %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, name, &width, &height, &target_bits, &c_min, &c_max,
                       &p[0], &p[1], &p[2], &p[3]) != 10) {
                fprintf(stderr, "bad target line\n");
                return 2;
            }
            float target;
            memcpy(&target, &target_bits, sizeof(target));
            if (!statmc::check_target_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), at<int32_t>(p[1]), target, c_min, c_max, at<int32_t>(p[2]),
                                           at<statmc_target_result>(p[3]), statmc::PlanMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::TargetArgs a;
                statmc::fill_target_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), at<int32_t>(p[1]), target, c_min, c_max, at<int32_t>(p[2]),
                                         at<statmc_target_result>(p[3]));
                printf("%s : ok target %lld %d %d\n", name, a.n_chunks, a.grid, a.vec);
            }
        } else {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
