// statmc_plan_args.h on its own: no library, no device, nothing but include/statmc.h.  Reads a table of calls -- the one
// tests/test_plan_cpu.py writes from its restatement of include/statmc.h -- and prints check_scores_call's / check_plan_call's verdict
// for each, and for the valid ones what fill_score_args / fill_plan_args made of them.  The image "pointers" of the table are numbers:
// nothing is read through them.
//
//   scores <name> <width> <height> <channels> <metric> <eps as float bits>  <n film_mean film_m2 score>
//   plan <name> <width> <height> <budget> <c_min> <c_max>  <score n sample_counts result workspace> <workspace_bytes>
//
// Output, one line per call:   <name> : ok scores <vec>   |   <name> : ok plan <workspace bytes> <chunks> <grid> <wide> <wide_wave> <vec>   |
//                              <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_plan_args.h"

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
        if (strcmp(word, "scores") == 0) {
            int channels, metric;
            uint32_t eps_bits;
            uint64_t p[4];
            if (fscanf(f, "%127s %d %d %d %d %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, name, &width, &height, &channels, &metric,
                       &eps_bits, &p[0], &p[1], &p[2], &p[3]) != 10) {
                fprintf(stderr, "bad scores line\n");
                return 2;
            }
            float eps;
            memcpy(&eps, &eps_bits, sizeof(eps));
            if (!statmc::check_scores_call((uint16_t)width, (uint16_t)height, channels, metric, eps, at<int32_t>(p[0]), at<float>(p[1]), at<float>(p[2]),
                                           at<float>(p[3]), statmc::PlanMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::ScoreArgs a;
                statmc::fill_score_args(a, (uint16_t)width, (uint16_t)height, channels, metric, eps, at<int32_t>(p[0]), at<float>(p[1]), at<float>(p[2]),
                                        at<float>(p[3]));
                printf("%s : ok scores %d\n", name, a.vec);
            }
        } else if (strcmp(word, "plan") == 0) {
            long long budget;
            int c_min, c_max;
            uint64_t p[5], ws_bytes;
            if (fscanf(f, "%127s %d %d %lld %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, name, &width, &height, &budget,
                       &c_min, &c_max, &p[0], &p[1], &p[2], &p[3], &p[4], &ws_bytes) != 12) {
                fprintf(stderr, "bad plan line\n");
                return 2;
            }
            if (!statmc::check_plan_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), at<int32_t>(p[1]), budget, c_min, c_max, at<int32_t>(p[2]),
                                         at<statmc_plan_result>(p[3]), at<void>(p[4]), (size_t)ws_bytes, statmc::PlanMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::PlanArgs a;
                statmc::fill_plan_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), at<int32_t>(p[1]), budget, c_min, c_max, at<int32_t>(p[2]),
                                       at<statmc_plan_result>(p[3]), at<void>(p[4]));
                printf("%s : ok plan %zu %lld %d %d %d %d\n", name, statmc::plan_workspace_bytes((uint16_t)width, (uint16_t)height), a.n_chunks, a.grid,
                       a.wide, a.wide_wave, a.vec);
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
