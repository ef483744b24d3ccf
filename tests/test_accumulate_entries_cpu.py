"""Every accumulation entry of include/statmc.h before statmc_setup, without a GPU: a table of malformed and valid calls on made-up addresses
(nothing launches without a device), each with the code it returns and which argument its message names.  What is expected,
tests/golden/accumulate_entries_nodevice.json, was recorded from the library as it was before the entries shared one argument
check (run this file as a script, in a checkout of that commit, to record it again): a call's code never depended on whether
its device had been set up, and which check answers first is part of the ABI.  Where a limit on n_types x n_ranges is the
answer the message may name n_ranges although the recorded one did not: the entries now share one text for it."""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "accumulate_entries_nodevice.json")
WORDS = ["n_types", "n_ranges", "n_tiles", "sample_formats", "sample_counts", "odd address", "n_records", "split_above", "stride", "types["]
F32, F16 = 0, 1
COUNTS = 0x7000

# entry -> the optional arguments it takes
FILM = {"statmc_accumulate": "", "statmc_accumulate_rows": "", "statmc_accumulate_row_ranges": "r", "statmc_accumulate_formats": "rf",
        "statmc_accumulate_counted": "rfc"}
TILES = {"statmc_accumulate_tiles": "t", "statmc_accumulate_tiles_formats": "tf", "statmc_accumulate_tiles_counted": "tfc"}
RECORDS = {"statmc_accumulate_records": "n", "statmc_accumulate_records_split": "ns", "statmc_accumulate_records_interleaved": "nl",
           "statmc_accumulate_records_interleaved_split": "nls"}
ENTRIES = dict(FILM, **dict(TILES, **RECORDS))


def stat_types(api, n, samples=0x1000):
    """Descriptors that pass every host-side check (no call here gets as far as reading through them)."""
    types = (api.StatType * max(n, 1))()
    for t in types:
        t.channels, t.transform, t.max_moment, t.n_samples = 3, 0, 1, 4
        t.samples, t.n, t.mean = samples, 0x2000, 0x3000
    return types


def call(lib, api, entry, n_types=2, types="ok", formats=None, counts=None, ranges=(0, 8), n_ranges=1, n_tiles=1, n_records=100,
         split_above=8, stride=16):
    """One call of `entry` on an 8 x 8 film; arguments the entry does not take are left out."""
    if types == "ok":
        types = stat_types(api, 17)
    elif types == "odd":
        types = stat_types(api, 17, samples=0x1001)
    fmts = (C.c_int32 * 17)(*formats) if formats is not None else None
    rng = (C.c_int32 * 32)(*ranges) if ranges is not None else None
    f = getattr(lib, entry)
    if entry == "statmc_accumulate":
        return f(8, 8, types, n_types, None)
    if entry == "statmc_accumulate_rows":
        return f(8, 8, types, n_types, 0, 8, None)
    if entry == "statmc_accumulate_row_ranges":
        return f(8, 8, types, n_types, rng, n_ranges, None)
    if entry == "statmc_accumulate_formats":
        return f(8, 8, types, fmts, n_types, rng, n_ranges, None)
    if entry == "statmc_accumulate_counted":
        return f(8, 8, types, fmts, n_types, counts, rng, n_ranges, None)
    if entry == "statmc_accumulate_tiles":
        return f(8, 8, types, n_types, 0x4000, 0x5000, 0x6000, n_tiles, None)
    if entry == "statmc_accumulate_tiles_formats":
        return f(8, 8, types, fmts, n_types, 0x4000, 0x5000, 0x6000, n_tiles, None)
    if entry == "statmc_accumulate_tiles_counted":
        return f(8, 8, types, fmts, n_types, 0x4000, 0x5000, 0x6000, n_tiles, counts, None)
    layout = api.make_record_layout(stride, 0, [4] * 16)
    tail = (split_above, None) if entry.endswith("_split") else (None,)
    if "interleaved" in entry:
        return f(8, 8, types, n_types, 0x10000, C.byref(layout), n_records, *tail)
    return f(8, 8, types, n_types, 0x8000, n_records, *tail)


def cases():
    """(name, entry, keyword arguments of call()), in a fixed order."""
    out = []
    # the calls whose codes the ABI's history fixed one by one
    seventeen_f32 = [F32] * 17
    out += [
        ("accumulate, n_types 17", "statmc_accumulate", dict(n_types=17)),
        ("formats, formats NULL, n_types 17", "statmc_accumulate_formats", dict(n_types=17)),
        ("formats, 17 x F32, n_types 17", "statmc_accumulate_formats", dict(n_types=17, formats=seventeen_f32)),
        ("formats (F32, F32), types NULL", "statmc_accumulate_formats", dict(formats=[F32, F32], types=None)),
        ("formats (F32, F16), types NULL", "statmc_accumulate_formats", dict(formats=[F32, F16], types=None)),
        ("counted, types NULL", "statmc_accumulate_counted", dict(counts=COUNTS, types=None)),
        ("counted, n_types 0", "statmc_accumulate_counted", dict(counts=COUNTS, n_types=0)),
        ("tiles, n_tiles -1", "statmc_accumulate_tiles", dict(n_tiles=-1)),
        ("tiles_formats (one half arena), n_tiles -1", "statmc_accumulate_tiles_formats", dict(formats=[F32, F16], n_tiles=-1)),
        ("tiles_counted, n_tiles -1", "statmc_accumulate_tiles_counted", dict(counts=COUNTS, n_tiles=-1)),
        ("tiles_counted, tile_bounds NULL", None, None),       # (a call of its own, below: call() always passes the bounds)
        ("records, n_types 17", "statmc_accumulate_records", dict(n_types=17)),
        ("records, types NULL", "statmc_accumulate_records", dict(types=None)),
    ]
    # every entry, in every combination of the optional arguments it takes, against every malformed argument it takes
    for entry, takes in ENTRIES.items():
        modes = [("", {})]
        if "f" in takes:
            modes = [("no formats", {}), ("f32", dict(formats=[F32] * 17)), ("a half", dict(formats=[F32, F16] + [F32] * 15))]
        if "c" in takes:
            modes = [(m + ", " + c, dict(kw, **ckw)) for m, kw in modes for c, ckw in (("no counts", {}), ("counts", dict(counts=COUNTS)))]
        for mode, base in modes:
            def add(what, **kw):
                out.append(("%s [%s] %s" % (entry[len("statmc_accumulate"):].lstrip("_") or "accumulate", mode, what), entry, dict(base, **kw)))
            add("valid")
            add("n_types -1", n_types=-1)
            add("n_types 17", n_types=17)
            add("n_types 0", n_types=0)
            add("types NULL", types=None)
            if "f" in takes:
                add("bad format first", formats=[2, F16])
                add("bad format last", formats=[F16, -1])
                add("odd half arena", formats=[F32, F16], types="odd")
                add("odd fp32 arena", formats=[F32, F32], types="odd")
            if "c" in takes:
                for k in (1, 2, 3):
                    add("counts + %d" % k, counts=COUNTS + k)
            if "r" in takes:
                add("n_ranges -1", n_ranges=-1)
                add("n_ranges 2, ranges NULL", ranges=None, n_ranges=2)
                add("n_ranges 0, ranges NULL", ranges=None, n_ranges=0)
                add("2 types x 9 ranges", ranges=[v for r in range(9) for v in (r % 8, r % 8)], n_ranges=9)
                add("17 types x 0 ranges", n_types=17, n_ranges=0)
            if "t" in takes:
                add("n_tiles -1", n_tiles=-1)
                add("n_tiles 0", n_tiles=0)
            if "n" in takes:
                add("n_records -1", n_records=-1)
                add("n_records 2^31", n_records=2 ** 31)
            if "s" in takes:
                add("split_above 0", split_above=0)
            if "l" in takes:
                add("stride 6", stride=6)
    return out


def answers(lib, api):
    """[name, code, the WORDS its message holds] per case."""
    out = []
    for name, entry, kw in cases():
        if entry is None:
            rc = lib.statmc_accumulate_tiles_counted(8, 8, stat_types(api, 2), None, 2, None, 0x5000, 0x6000, 1, COUNTS, None)
        else:
            rc = call(lib, api, entry, **kw)
        msg = lib.statmc_last_error().decode()
        out.append([name, rc, [w for w in WORDS if w in msg] if rc != api.ERR_NO_DEVICE else []])
    return out


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_the_table_covers_every_entry():
    from statmc_amd import api
    declared = re.findall(r"^int\s+(statmc_accumulate\w*)\s*\(", open(os.path.join(ROOT, "include", "statmc.h")).read(), re.M)
    assert sorted(declared) == sorted(ENTRIES) and all(e in api.EXPORTS for e in ENTRIES)
    names = [c[0] for c in cases()]
    assert len(set(names)) == len(names)
    want = json.load(open(GOLDEN))["cases"]
    assert [w[0] for w in want] == names, "the case list and the golden file's differ"
    assert os.path.getsize(GOLDEN) < 128 * 1024


def test_every_call_answers_as_recorded():
    if not _no_gpu():
        pytest.skip("a GPU is present")       # the valid calls would run on made-up addresses
    from statmc_amd import api
    lib = api.load()
    want = json.load(open(GOLDEN))["cases"]
    got = answers(lib, api)
    wrong = []
    for (name, rc, words), (_, want_rc, want_words) in zip(got, want):
        extra = set(words) - set(want_words)
        if rc != want_rc or not set(want_words) <= set(words) or not extra <= {"n_ranges"}:
            wrong.append((name, (rc, words), (want_rc, want_words)))
    assert not wrong, "%d of %d calls, the first (name, got, recorded): %s" % (len(wrong), len(want), wrong[0])
    assert lib.statmc_debug_last_accumulate_counted() == 0


def test_the_recorded_answers_hold_the_documented_ones():
    """The codes the ABI's history fixed, written out here: -4 STATMC_ERR_NO_DEVICE, -1 STATMC_ERR_INVALID."""
    want = {w[0]: (w[1], w[2]) for w in json.load(open(GOLDEN))["cases"]}
    table = [("accumulate, n_types 17", -4, None), ("formats, formats NULL, n_types 17", -4, None), ("formats, 17 x F32, n_types 17", -1, "n_types"),
             ("formats (F32, F32), types NULL", -4, None), ("formats (F32, F16), types NULL", -1, None), ("counted, types NULL", -1, None),
             ("counted, n_types 0", -4, None), ("tiles, n_tiles -1", -4, None), ("tiles_formats (one half arena), n_tiles -1", -4, None),
             ("tiles_counted, n_tiles -1", -1, "n_tiles"), ("tiles_counted, tile_bounds NULL", -4, None), ("records, n_types 17", -1, "n_types"),
             ("records, types NULL", -4, None)]
    for name, code, word in table:
        assert want[name][0] == code and (word is None or word in want[name][1]), (name, want[name])
    assert all(rc in (-1, -4) for rc, _ in want.values())      # nothing succeeds, and nothing launches, without a device


if __name__ == "__main__":      # record GOLDEN's content from the library of this checkout: python tests/test_accumulate_entries_cpu.py OUT.json
    sys.path.insert(0, ROOT)
    from statmc_amd import api as _api
    assert _no_gpu()
    with open(sys.argv[1], "w") as out:
        out.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in answers(_api.load(), _api)) + "\n]}\n")
