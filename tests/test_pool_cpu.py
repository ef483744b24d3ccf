"""statmc_pool_statistics (include/statmc.h) without a GPU: the symbol, its declaration and the ctypes mirror; the argument checks of
statmc_amd/csrc/statmc_pool_args.h -- compiled alone into tests/cpp/test_pool_args.cpp, plain and under AddressSanitizer and UBSan --
against a Python restatement of the header's rules; what the built library answers without a device; and a numpy float32
restatement of the Morton-ordered tree: its composition property and its distance from the union of the samples."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_combine_cpu import two_pass64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_pool_args.cpp")
KS = (2, 4, 8)
PLANES = ("n", "mean", "m2", "m3", "film_mean", "film_m2", "mean_corr", "discriminator")
FW, FH = 64, 48                  # the film of the table's calls
STEP = 1 << 20                   # made-up images lie 1 MiB apart: the largest plane of the table has 64 * 48 * 3 * 4 = 36864 bytes


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- the table of calls and the restatement of include/statmc.h
def side(base, ch=3, mm=3, n=True, film=True, epilogue=False):
    """one statmc_stat_type of made-up addresses: the images of a side lie STEP apart, n first"""
    s = dict(channels=ch, max_moment=mm, **{p: 0 for p in PLANES})
    for i, p in enumerate(PLANES):
        have = {"n": n, "mean": True, "m2": mm >= 2, "m3": mm >= 3, "film_mean": film, "film_m2": film,
                "mean_corr": epilogue, "discriminator": epilogue}[p]
        s[p] = base + i * STEP if have else 0
    return s


def entry(i, count_of=-1, **kw):
    """entry i: dst at (2 i + 1) * 16 MiB, src at (2 i + 2) * 16 MiB"""
    dst_kw = dict(kw)
    src_kw = {k: v for k, v in kw.items() if k != "epilogue"}
    return dict(count_of=count_of, dst=side((2 * i + 1) * 16 * STEP, **dst_kw), src=side((2 * i + 2) * 16 * STEP, **src_kw))


def call(entries, width=FW, height=FH, k=2, n_entries=None, given=True):
    return dict(width=width, height=height, k=k, n_entries=len(entries) if n_entries is None else n_entries, given=given, entries=entries)


def film_set(epilogue=True):
    """radiance with counts, film images and the epilogue; the "film" image and a 1-channel mean that borrow its counts"""
    return [entry(0, epilogue=epilogue), entry(1, count_of=0, mm=1, n=False, film=False), entry(2, count_of=0, ch=1, mm=1, n=False, film=False)]


def edited(entries, i, which, **fields):
    entries[i][which].update(fields)
    return entries


def coarse(v, k):
    return -(-v // k)


def table():
    t = {}
    for k in KS:
        t["valid_k%d" % k] = call(film_set(), k=k)
        t["valid_odd_film_k%d" % k] = call(film_set(), width=61, height=47, k=k)
    t["valid_no_entries"] = call([], n_entries=0, given=False)
    t["valid_sixteen_entries"] = call([entry(i, mm=1, film=False) for i in range(16)])
    e = film_set()
    e[1]["dst"].update(film_mean=e[1]["dst"]["mean"]), e[1]["src"].update(film_mean=e[1]["src"]["mean"])     # aliased: pooled once
    t["valid_film_planes_alias_the_moments"] = call(e)
    t["valid_film_mean_only"] = call(edited(edited(film_set(False), 0, "dst", film_m2=0), 0, "src", film_m2=0))
    t["valid_unaligned_plane"] = call(edited(film_set(), 0, "src", m2=2 * 16 * STEP + 2 * STEP + 4))
    for k in (0, 1, 3, 16, -2):
        t["bad_k_%d" % k] = call(film_set(), k=k)
    t["zero_width"] = call(film_set(), width=0)
    t["zero_height"] = call(film_set(), height=0)
    t["seventeen_entries"] = call([entry(i, mm=1, film=False) for i in range(17)])
    t["negative_n_entries"] = call(film_set(), n_entries=-1)
    t["null_entries"] = call([], n_entries=2, given=False)
    t["channels_2"] = call([entry(0, ch=2)])
    t["max_moment_0"] = call([entry(0, mm=0)])
    t["max_moment_4"] = call([entry(0, mm=4)])
    t["src_channels_differ"] = call(edited(film_set(), 0, "src", channels=1))
    t["src_max_moment_differs"] = call(edited(film_set(), 0, "src", max_moment=2))
    t["src_without_film_planes"] = call(edited(film_set(), 0, "src", film_mean=0, film_m2=0))
    t["dst_without_film_m2"] = call(edited(film_set(False), 0, "dst", film_m2=0))
    t["film_m2_without_film_mean"] = call(edited(edited(film_set(), 0, "dst", film_mean=0), 0, "src", film_mean=0))
    for p in ("mean", "m2", "m3"):
        t["null_dst_" + p] = call(edited(film_set(), 0, "dst", **{p: 0}))
        t["null_src_" + p] = call(edited(film_set(), 0, "src", **{p: 0}))
    t["null_dst_n"] = call(edited(film_set(), 0, "dst", n=0))
    t["null_src_n"] = call(edited(film_set(), 0, "src", n=0))
    e = film_set()
    e[1]["count_of"] = 3
    t["count_of_past_the_entries"] = call(e)
    e = film_set()
    e[1]["count_of"] = 1
    t["count_of_itself"] = call(e)
    e = film_set()
    e[2]["count_of"] = 1
    t["count_of_a_borrower"] = call(e)
    e = film_set()
    e[1]["count_of"] = -2
    t["count_of_minus_2"] = call(e)
    t["borrower_with_dst_n"] = call(edited(film_set(), 1, "dst", n=5 * 16 * STEP + 40 * STEP))
    t["borrower_with_src_n"] = call(edited(film_set(), 1, "src", n=5 * 16 * STEP + 40 * STEP))
    t["mean_corr_alone"] = call(edited(film_set(), 0, "dst", discriminator=0))
    t["discriminator_alone"] = call(edited(film_set(), 0, "dst", mean_corr=0))
    t["epilogue_with_max_moment_2"] = call([entry(0, mm=2, epilogue=True)])
    t["epilogue_with_borrowed_counts"] = call(edited(film_set(), 1, "dst", mean_corr=5 * 16 * STEP + 41 * STEP, discriminator=5 * 16 * STEP + 42 * STEP))
    # byte ranges: a dst plane has the coarse size, a src plane the fine one
    src0 = film_set()[0]["src"]
    fine3, fine1 = FW * FH * 3 * 4, FW * FH * 4
    for k in KS:
        c3, c1 = coarse(FW, k) * coarse(FH, k) * 3 * 4, coarse(FW, k) * coarse(FH, k) * 4
        t["dst_mean_is_src_mean_k%d" % k] = call(edited(film_set(), 0, "dst", mean=src0["mean"]), k=k)
        t["dst_m2_in_the_last_bytes_of_src_m3_k%d" % k] = call(edited(film_set(), 0, "dst", m2=src0["m3"] + fine3 - 4), k=k)
        t["valid_dst_m2_right_behind_src_m3_k%d" % k] = call(edited(film_set(), 0, "dst", m2=src0["m3"] + fine3), k=k)
        t["dst_m3_ends_inside_src_mean_k%d" % k] = call(edited(film_set(), 0, "dst", m3=src0["mean"] - c3 + 4), k=k)
        t["valid_dst_m3_ends_at_src_mean_k%d" % k] = call(edited(film_set(), 0, "dst", m3=src0["mean"] - c3), k=k)
        t["dst_n_ends_inside_src_n_k%d" % k] = call(edited(film_set(), 0, "dst", n=src0["n"] - c1 + 4), k=k)
        t["valid_dst_n_ends_at_src_n_k%d" % k] = call(edited(film_set(), 0, "dst", n=src0["n"] - c1), k=k)
        t["borrower_dst_over_the_owners_src_n_k%d" % k] = call(edited(film_set(), 1, "dst", mean=src0["n"] + fine1 - 4), k=k)
        t["dst_mean_corr_over_another_entrys_src_k%d" % k] = call(edited(film_set(), 0, "dst", mean_corr=film_set()[2]["src"]["mean"] + fine1 - 4), k=k)
    t["two_entries_write_one_dst_plane"] = call(edited(film_set(), 2, "dst", mean=film_set()[0]["dst"]["m2"]))
    e = [entry(0), entry(1)]
    e[1]["dst"]["n"] = e[0]["dst"]["n"]
    t["two_entries_own_one_count_image"] = call(e)
    return t


def own_film(s):
    fm = s["film_mean"] != 0 and s["film_mean"] != s["mean"]
    f2 = s["film_m2"] != 0 and s["film_m2"] != s["m2"]
    return fm, f2


def planes_of(s, dst, own, n_px):
    """[(name, address, bytes)] of the images of one side that the call moves"""
    fm, f2 = own_film(s)
    img = n_px * s["channels"] * 4
    out = [("mean", s["mean"], img)]
    if s["max_moment"] >= 2:
        out.append(("m2", s["m2"], img))
    if s["max_moment"] >= 3:
        out.append(("m3", s["m3"], img))
    if fm:
        out.append(("film_mean", s["film_mean"], img))
    if f2:
        out.append(("film_m2", s["film_m2"], img))
    if own:
        out.append(("n", s["n"], n_px * 4))
    if dst:
        out += [(p, s[p], img) for p in ("mean_corr", "discriminator")]
    return [p for p in out if p[1] != 0]


def restated(c):
    """include/statmc.h's error list for statmc_pool_statistics: None for a valid call, else words the message must contain"""
    if c["k"] not in KS:
        return ["k = %d" % c["k"]]
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    if not 0 <= c["n_entries"] <= 16:
        return ["n_entries"]
    if c["n_entries"] == 0:
        return None
    if not c["given"]:
        return ["null entries"]
    es = c["entries"][:c["n_entries"]]
    for i, e in enumerate(es):
        d, s, who = e["dst"], e["src"], "entries[%d]" % i
        if d["channels"] not in (1, 3):
            return [who, "channels"]
        if not 1 <= d["max_moment"] <= 3:
            return [who, "max_moment"]
        if (s["channels"], s["max_moment"]) != (d["channels"], d["max_moment"]):
            return [who, "dst and src disagree"]
        q = e["count_of"]
        if q == -1:
            if not d["n"] or not s["n"]:
                return [who, "null n"]
        elif q < 0 or q >= len(es) or q == i or es[q]["count_of"] != -1:
            return [who, "count_of"]
        elif d["n"] or s["n"]:
            return [who, "dst.n and src.n must be NULL"]
        for x in (d, s):
            fm, f2 = own_film(x)
            if f2 and not fm:
                return [who, "film_m2 without a film_mean"]
        if own_film(d) != own_film(s):
            return [who, "film planes"]
        for f in ("mean", "m2", "m3")[:d["max_moment"]]:
            if not d[f] or not s[f]:
                return [who, "null " + f]
        if d["mean_corr"] or d["discriminator"]:
            if not d["mean_corr"] or not d["discriminator"]:
                return [who, "mean_corr and discriminator"]
            if d["max_moment"] < 3:
                return [who, "max_moment 3"]
            if q != -1:
                return [who, "counts of the entry's own"]
    fine, crs = c["width"] * c["height"], coarse(c["width"], c["k"]) * coarse(c["height"], c["k"])
    for i, e in enumerate(es):
        mine = planes_of(e["dst"], True, e["count_of"] == -1, crs)
        for j, o in enumerate(es):
            theirs = planes_of(o["dst"], True, o["count_of"] == -1, crs)
            for name, p, nb in mine:
                if j < i:
                    for oname, op, _ in theirs:
                        if p == op:
                            return ["entries[%d] and [%d]" % (j, i), "count image" if name == oname == "n" else "same dst image"]
                for _, sp, sb in planes_of(o["src"], False, o["count_of"] == -1, fine):
                    if p < sp + sb and sp < p + nb:
                        return ["entries[%d]" % i, "overlaps a src image of entries[%d]" % j]
    return None


def write_table(path, calls):
    with open(path, "w") as f:
        for name, c in calls.items():
            f.write("call %s %d %d %d %d %d %d\n" % (name, c["width"], c["height"], c["k"], c["n_entries"], int(c["given"]), len(c["entries"])))
            for e in c["entries"]:
                words = [str(e["count_of"])]
                for s in (e["dst"], e["src"]):
                    words += [str(s["channels"]), str(s["max_moment"])] + [str(s[p]) for p in PLANES]
                f.write("entry " + " ".join(words) + "\n")


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("pool") / "table.txt")
    write_table(path, table())
    return path, verdicts(build.POOL_ARGS_BIN, path)


# ---------------------------------------------------------------- 1. the args header, alone
def test_the_table_states_every_error_once_and_valid_calls_for_each_k():
    t = table()
    want = {name: restated(c) for name, c in t.items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid_"), (name, w)
    for k in KS:
        assert want["valid_k%d" % k] is None
    said = set(" ".join(w[-1:]) for w in want.values() if w)
    assert len(said) >= 20, sorted(said)          # the error list of include/statmc.h, each rule with a message of its own


def test_the_args_header_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(t)
    for name, c in t.items():
        want = restated(c)
        if want is None:
            assert got[name].startswith("ok "), (name, got[name])
            words = got[name].split()
            assert [int(w) for w in words[1:3]] == [coarse(c["width"], c["k"]), coarse(c["height"], c["k"])], name
            es = c["entries"][:c["n_entries"]]
            src_aligned = all(p % 8 == 0 for e in es for _, p, _ in planes_of(e["src"], False, False, 0))
            counts_aligned = all((e["src"]["n"] if e["count_of"] == -1 else es[e["count_of"]]["src"]["n"]) % 8 == 0 for e in es)
            assert int(words[3]) == int(c["width"] % 2 == 0 and src_aligned and counts_aligned), name
            per_entry = re.findall(r"\{(\d+) (\d+) (\d+) (\d+)\}", got[name])
            assert len(per_entry) == len(es)
            for e, (cnt_src, cnt_dst, moments, film) in zip(es, per_entry):
                owner = e if e["count_of"] == -1 else es[e["count_of"]]
                assert int(cnt_src) == owner["src"]["n"] and int(cnt_dst) == (e["dst"]["n"] if e["count_of"] == -1 else 0), name
                assert int(moments) == e["dst"]["max_moment"] and int(film) == sum(own_film(e["dst"])), name
        else:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "pool_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


# ---------------------------------------------------------------- 2. the library, without a device
def test_symbol_is_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build
    assert hasattr(lib, "statmc_pool_statistics") and "statmc_pool_statistics" in api.EXPORTS
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decl = re.search(r"int\s+statmc_pool_statistics\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, int k, const statmc_pool_entry *entries, "
                                                        "int n_entries, void *stream")
    pe, ce = api.PoolEntry, api.CombineEntry
    assert [C.sizeof(pe), pe.dst.offset, pe.src.offset, pe.count_of.offset] == [C.sizeof(ce), ce.dst.offset, ce.src.offset, ce.count_of.offset]
    assert re.search(r"typedef struct statmc_pool_entry \{\s*statmc_stat_type dst;[^}]*statmc_stat_type src;[^}]*int32_t count_of;[^}]*\} statmc_pool_entry;", header)
    assert "statmc_pool.hip" in build.SOURCES and "statmc_pool_args.h" in build.HEADERS
    assert api.pooled_size(7, 3, 2) == (4, 2) and api.pooled_size(18, 10, 8) == (3, 2) and api.pooled_size(1920, 1080, 8) == (240, 135)


def as_ctypes(api, c):
    arr = (api.PoolEntry * max(len(c["entries"]), 1))()
    for i, e in enumerate(c["entries"]):
        arr[i].count_of = e["count_of"]
        for which in ("dst", "src"):
            t = getattr(arr[i], which)
            t.channels, t.max_moment = e[which]["channels"], e[which]["max_moment"]
            for p in PLANES:
                setattr(t, p, e[which][p] or None)
    return arr


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every invalid call of the table is refused with its argument named whether or not a
    device is set up; n_entries = 0 is a no-op; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        arr = as_ctypes(api, c)
        if want is not None:
            assert lib.statmc_pool_statistics(c["width"], c["height"], c["k"], arr if c["given"] else None, c["n_entries"], None) == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif c["n_entries"] == 0:
            assert lib.statmc_pool_statistics(c["width"], c["height"], c["k"], None, 0, None) == api.STATMC_OK, name
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_pool_gpu.py runs real ones)
            assert lib.statmc_pool_statistics(c["width"], c["height"], c["k"], arr, c["n_entries"], None) == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- 3. the tree, restated in numpy float32
F32 = np.float32


def morton(j):
    """slot j -> (dx, dy): bit 2 i of j is bit i of dx, bit 2 i + 1 is bit i of dy"""
    dx = (j & 1) | ((j >> 1) & 2) | ((j >> 2) & 4)
    dy = ((j >> 1) & 1) | ((j >> 2) & 2) | ((j >> 3) & 4)
    return dx, dy


def merge32(A, B):
    """include/statmc.h's fp32 operation order, part B into part A (dicts: n int32 [H, W]; mean, m2, m3 float32 [H, W, C]); every
    numpy float32 operation rounds once, and x / nf is the correctly rounded quotient the device's division returns"""
    nA, nB = A["n"], B["n"]
    fA, fB, nf = nA.astype(F32)[..., None], nB.astype(F32)[..., None], (nA + nB).astype(F32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = B["mean"] - A["mean"]
        t = (d * fB) / nf
        q = d * fA
        u = d / nf
        qt = q * t
        f = {"mean": A["mean"] + t, "m2": (A["m2"] + B["m2"]) + qt,
             "m3": ((A["m3"] + B["m3"]) + qt * ((fA - fB) * u)) + (F32(3) * u) * (fA * B["m2"] - fB * A["m2"])}
    out = {"n": nA + nB}
    for k, v in f.items():
        assert v.dtype == F32
        out[k] = np.where((nB == 0)[..., None], A[k], np.where((nA == 0)[..., None], B[k], v))
    return out


def slots_of(film, k):
    """the k * k part states of the coarse size, slot j = Morton(dx, dy); a slot outside the film is the cleared state"""
    H, W = film["n"].shape
    Hc, Wc = coarse(H, k), coarse(W, k)
    parts = []
    for j in range(k * k):
        dx, dy = morton(j)
        part = {key: np.zeros((Hc, Wc) + v.shape[2:], v.dtype) for key, v in film.items()}
        ys, xs = np.arange(dy, H, k), np.arange(dx, W, k)
        for key, v in film.items():
            part[key][:len(ys), :len(xs)] = v[dy::k, dx::k]
        parts.append(part)
    return parts


def pool32(film, k):
    parts = slots_of(film, k)
    stride = 1
    while stride < k * k:
        for j in range(0, k * k, 2 * stride):
            parts[j] = merge32(parts[j], parts[j + stride])
        stride *= 2
    return parts[0]


def fold32(st, values, counts):
    """the sequential accumulation, fp32 (add_sample of include/statmc_device_api.hpp without the transform): values[s] into the
    pixels with s < counts, in ascending s"""
    for s in range(values.shape[0]):
        live = s < counts
        n = st["n"] + live
        nf = np.maximum(n, 1).astype(F32)[..., None]
        d = values[s] - st["mean"]
        dN = d / nf
        mean = st["mean"] + dN
        m2 = st["m2"] + d * (d - dN)
        m3 = st["m3"] + (F32(-3) * dN * m2 + d * (d * d - dN * dN))
        for key, v in (("mean", mean), ("m2", m2), ("m3", m3)):
            assert v.dtype == F32
            st[key] = np.where(live[..., None], v, st[key])
        st["n"] = n.astype(np.int32)
    return st


def cleared(H, W, ch):
    return {"n": np.zeros((H, W), np.int32), **{k: np.zeros((H, W, ch), F32) for k in ("mean", "m2", "m3")}}


def box_cox_samples(rng, S, H, W, ch):
    """Box-Cox'd log-normal samples, a per-pixel scale spread of e^+-1.5, 20 % zeros; 0 to S samples per pixel"""
    scale = np.exp(rng.uniform(-1.5, 1.5, (1, H, W, 1)))
    x = (np.exp(rng.normal(0.0, 1.0, (S, H, W, ch))) * scale).astype(F32)
    x *= rng.random((S, H, W, 1)) >= 0.2
    values = ((np.sqrt(x) - F32(1)) / F32(.5)).astype(F32)
    counts = rng.integers(0, S + 1, (H, W)).astype(np.int32)
    return values, counts


def same_bits(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k)
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), (what, k)


@pytest.mark.parametrize("W,H", [(7, 5), (8, 8), (18, 10)])
def test_restated_tree_composes_bit_for_bit(W, H):
    """pool_2(pool_2) == pool_4 and pool_2(pool_4) == pool_4(pool_2) == pool_2(pool_2(pool_2)) == pool_8: the Morton order makes the
    levels alternate x and y pairs, so a pooled film's tree is the upper part of the fine film's tree -- partial blocks included"""
    rng = np.random.default_rng(W * 100 + H)
    values, counts = box_cox_samples(rng, 18, H, W, 3)
    counts[rng.random((H, W)) < 0.3] = 0
    counts[0, 0] = 0
    counts[4:8, 4:8] = 0        # a whole block without a sample for k = 2 and k = 4 (a partial one on 7 x 5)
    fine = fold32(cleared(H, W, 3), values, counts)
    for k in fine:      # a payload in the pixels without samples: which empty slot's bits survive is part of the definition
        if k != "n":
            fine[k][counts == 0] = rng.normal(0, 1, fine[k][counts == 0].shape).astype(F32)
    p2, p4, p8 = pool32(fine, 2), pool32(fine, 4), pool32(fine, 8)
    same_bits(pool32(p2, 2), p4, "2 o 2 = 4")
    same_bits(pool32(p4, 2), p8, "2 o 4 = 8")
    same_bits(pool32(p2, 4), p8, "4 o 2 = 8")
    same_bits(pool32(pool32(p2, 2), 2), p8, "2 o 2 o 2 = 8")
    for k, p in ((2, p2), (4, p4), (8, p8)):
        sums = np.add.reduceat(np.add.reduceat(counts, np.arange(0, H, k), axis=0), np.arange(0, W, k), axis=1)
        assert np.array_equal(p["n"], sums), k
        empty = sums == 0
        assert empty.any() or k == 8
        assert (~empty).any()
        for f in ("mean", "m2", "m3"):       # an empty block keeps slot 0's bits
            assert np.array_equal(p[f][empty].view(np.int32), fine[f][::k, ::k][empty].view(np.int32)), (k, f)
    # ... which a row-major slot order would not give: the same tree over slots j = dy * k + dx
    def row_major(film, k):
        parts = slots_of(film, k)
        order = [next(j for j in range(k * k) if morton(j) == (i % k, i // k)) for i in range(k * k)]
        parts = [parts[j] for j in order]
        stride = 1
        while stride < k * k:
            for j in range(0, k * k, 2 * stride):
                parts[j] = merge32(parts[j], parts[j + stride])
            stride *= 2
        return parts[0]
    rm4 = row_major(fine, 4)      # (for k = 2 the two orders are the same four slots: pooling by 2 twice is p4 either way)
    assert np.array_equal(rm4["n"], p4["n"])
    assert any(not np.array_equal(p4[f].view(np.int32), rm4[f].view(np.int32)) for f in ("mean", "m2", "m3"))


@pytest.mark.parametrize("k", KS)
def test_restated_tree_stays_inside_the_union_rule(k):
    """check_union_rule of tests/test_device_reduce_gpu.py: per field at most twice as far (relative L2) from the float64 two-pass
    moments of the block's samples as the sequential fp32 fold of the same samples in slot order, + 1e-6"""
    from test_device_reduce_gpu import check_union_rule
    rng = np.random.default_rng(77 + k)
    S, W, H, ch = 18, 44, 27, 3
    values, counts = box_cox_samples(rng, S, H, W, ch)
    fine = fold32(cleared(H, W, ch), values, counts)
    got = pool32(fine, k)
    Hc, Wc = coarse(H, k), coarse(W, k)
    seq = cleared(Hc, Wc, ch)
    ref = {f: np.zeros((Hc, Wc, ch)) for f in ("mean", "m2", "m3")}
    padded_v = np.zeros((S, Hc * k, Wc * k, ch), F32)
    padded_v[:, :H, :W] = values
    padded_c = np.zeros((Hc * k, Wc * k), np.int32)
    padded_c[:H, :W] = counts
    for j in range(k * k):
        dx, dy = morton(j)
        seq = fold32(seq, padded_v[:, dy::k, dx::k], padded_c[dy::k, dx::k])
    for Y in range(Hc):
        for X in range(Wc):
            block_v, block_c = padded_v[:, Y * k:(Y + 1) * k, X * k:(X + 1) * k], padded_c[Y * k:(Y + 1) * k, X * k:(X + 1) * k]
            live = np.arange(S)[:, None, None] < block_c[None]
            if live.any():
                ref["mean"][Y, X], ref["m2"][Y, X], ref["m3"][Y, X] = two_pass64(block_v[live])
    assert np.array_equal(got["n"], seq["n"]) and got["n"].sum() == counts.sum()
    check_union_rule(got, seq, ref, ("mean", "m2", "m3"), "restated tree, k = %d" % k)
