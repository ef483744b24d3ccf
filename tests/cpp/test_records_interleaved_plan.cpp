// statmc_records_plan.h without a device and without the library: which fold plan_records_interleaved picks for a list of type sets
// and formats, and what check_records_interleaved says to a list of layouts.  One line per case, which
// tests/test_records_interleaved_cpu.py compares with what it expects:
//   plan <name> : path K M fmt order...          (path 1 general, 2 fused)
//   check <name> : ok | <the message>
// The pointers are made up; nothing is dereferenced but the descriptors and the layout.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../statmc_amd/csrc/statmc_records_plan.h"

using namespace statmc;

namespace {

struct Kind { int channels, transform, max_moment; };
const Kind RAD{3, 1, 3}, RGB{3, 0, 1}, F1{1, 0, 1}, X2{1, 1, 2};

std::vector<statmc_stat_type> typesOf(const std::vector<Kind> &kinds) {
    std::vector<statmc_stat_type> out;
    for (const Kind &k : kinds) {
        statmc_stat_type t{};
        t.channels = k.channels;
        t.transform = k.transform;
        t.max_moment = k.max_moment;
        out.push_back(t);
    }
    return out;
}

// the fields behind the pixel index in the order given, each at the next multiple of its element size; stride rounded up to 4
statmc_record_layout tight(const std::vector<Kind> &kinds, const std::vector<int> &formats) {
    statmc_record_layout l{};
    int at = 4;
    for (size_t i = 0; i < kinds.size(); i++) {
        const int fmt = i < formats.size() ? formats[i] : STATMC_SAMPLES_F32;
        const int elem = fmt == STATMC_SAMPLES_F16 ? 2 : 4;
        at = (at + elem - 1) / elem * elem;
        l.sample_offset[i] = at;
        l.sample_format[i] = fmt;
        at += kinds[i].channels * elem;
    }
    l.stride = (at + 3) / 4 * 4;
    return l;
}

void plan(const char *name, const std::vector<Kind> &kinds, const statmc_record_layout &l, int force) {
    const std::vector<statmc_stat_type> types = typesOf(kinds);
    char msg[256] = "";
    if (!check_records_interleaved(types.data(), (int)types.size(), reinterpret_cast<const void *>(0x1000), &l, 100, msg, sizeof(msg))) {
        std::printf("plan %s : invalid: %s\n", name, msg);
        return;
    }
    const RecordsInterleavedPlan p = plan_records_interleaved(types.data(), (int)types.size(), l, force);
    std::printf("plan %s : %d %d %d %d", name, p.path, p.K, p.M, p.fmt);
    if (p.path == kRecIlvFused)
        for (int j = 0; j < 1 + p.K + p.M; j++) std::printf(" %d", p.order[j]);
    std::printf("\n");
}

void check(const char *name, const std::vector<Kind> &kinds, const void *records, const statmc_record_layout *l, int64_t n_records, int n_types = -100) {
    const std::vector<statmc_stat_type> types = typesOf(kinds);
    char msg[256] = "";
    const bool ok = check_records_interleaved(types.empty() ? nullptr : types.data(), n_types == -100 ? (int)types.size() : n_types, records, l, n_records,
                                              msg, sizeof(msg));
    std::printf("check %s : %s\n", name, ok ? "ok" : msg);
}

}  // namespace

int main() {
    const int F32 = STATMC_SAMPLES_F32, F16 = STATMC_SAMPLES_F16;
    const std::vector<Kind> five{RAD, RGB, RGB, F1, F1};
    // ---- the path
    plan("five f32", five, tight(five, {}), 0);
    plan("five feat16", five, tight(five, {F32, F16, F16, F16, F16}), 0);
    plan("five all16", five, tight(five, {F16, F16, F16, F16, F16}), 0);
    plan("five rad16 only", five, tight(five, {F16, F32, F32, F32, F32}), 0);
    plan("five mixed features", five, tight(five, {F32, F16, F32, F16, F16}), 0);
    plan("five f32 forced general", five, tight(five, {}), 1);
    plan("five f32 forced fused", five, tight(five, {}), 2);
    plan("five shuffled types", {F1, RGB, RAD, F1, RGB}, tight({F1, RGB, RAD, F1, RGB}, {}), 0);
    plan("one type", {RAD}, tight({RAD}, {}), 0);
    plan("one type forced fused", {RAD}, tight({RAD}, {}), 2);
    plan("three", {RAD, RGB, RGB}, tight({RAD, RGB, RGB}, {}), 0);
    plan("rad+f1", {RAD, F1}, tight({RAD, F1}, {}), 0);
    plan("features only", {RGB, F1}, tight({RGB, F1}, {}), 2);
    plan("two radiance", {RAD, RAD}, tight({RAD, RAD}, {}), 2);
    plan("three rgb", {RAD, RGB, RGB, RGB}, tight({RAD, RGB, RGB, RGB}, {}), 2);
    plan("tests' four", {RAD, RGB, F1, X2}, tight({RAD, RGB, F1, X2}, {}), 2);
    {
        std::vector<Kind> sixteen(16, F1);
        sixteen[0] = RAD;
        plan("sixteen", sixteen, tight(sixteen, {}), 0);
        plan("sixteen forced fused", sixteen, tight(sixteen, {}), 2);
    }
    {   // overlapping fields: the radiance field feeds the transform type and a plain RGB type; a 1-channel type reads its first channel
        statmc_record_layout l{};
        l.stride = 16;
        l.sample_offset[0] = l.sample_offset[1] = l.sample_offset[2] = 4;
        plan("overlap rad+rgb+f1", {RAD, RGB, F1}, l, 0);
        plan("overlap two radiance", {RAD, RAD}, l, 0);
    }
    // ---- the limits and the layout rules
    const void *rec = reinterpret_cast<const void *>(0x1000);
    statmc_record_layout ok = tight(five, {});
    check("tight 48", five, rec, &ok, 100);
    check("n_types 17", five, rec, &ok, 100, 17);
    check("n_types -1", five, rec, &ok, 100, -1);
    check("n_records -1", five, rec, &ok, -1);
    check("n_records 2^31", five, rec, &ok, (int64_t)1 << 31);
    check("n_records 2^31 - 1", five, rec, &ok, ((int64_t)1 << 31) - 1);
    check("null layout, nothing to do", {}, nullptr, nullptr, 0);
    check("null layout, records", {}, rec, nullptr, 5);
    check("null layout, types", five, rec, nullptr, 0);
    check("null types", {}, rec, &ok, 5, 2);
    check("records + 2", five, reinterpret_cast<const void *>(0x1002), &ok, 100);
    check("records + 4", five, reinterpret_cast<const void *>(0x1004), &ok, 100);
    auto with = [&](auto change) {
        statmc_record_layout l = ok;
        change(l);
        return l;
    };
    statmc_record_layout l;
    l = with([](statmc_record_layout &x) { x.stride = 0; });
    check("stride 0", {}, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.stride = -48; });
    check("stride -48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.stride = 50; });
    check("stride 50", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.stride = 4; });
    check("stride 4, no types", {}, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.pixel_offset = -4; });
    check("pixel_offset -4", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.pixel_offset = 2; });
    check("pixel_offset 2", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.pixel_offset = 48; });
    check("pixel_offset 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.pixel_offset = 44; });
    check("pixel_offset 44", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[1] = -4; });
    check("offset -4", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[1] = 6; });
    check("f32 offset 6", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[1] = 40; });
    check("rgb f32 at 40 of 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[1] = 36; });
    check("rgb f32 at 36 of 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[4] = 48; });
    check("f1 f32 at 48 of 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_offset[1] = 0x7ffffffc; });
    check("offset near 2^31", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[2] = F16; x.sample_offset[2] = 7; });
    check("half offset 7", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[2] = F16; x.sample_offset[2] = 6; });
    check("half offset 6", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[2] = F16; x.sample_offset[2] = 44; });
    check("rgb half at 44 of 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[2] = F16; x.sample_offset[2] = 42; });
    check("rgb half at 42 of 48", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[3] = 2; });
    check("format 2", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[0] = -1; });
    check("format -1", five, rec, &l, 5);
    l = with([](statmc_record_layout &x) { x.sample_format[7] = 9; x.sample_offset[7] = -3; });     // behind n_types: not looked at
    check("garbage behind n_types", five, rec, &l, 5);
    check("channels 2", {RAD, Kind{2, 0, 1}}, rec, &ok, 5);
    return 0;
}
