"""Packed scenes: save, load and append the 16-byte chunked splat format (include/gsplat/gs_abi.h "packed scenes").

The reference every answer is held to is tests/pack_restate.py, the numpy restatement of the header's definition: the codec, the
Morton order and the file.  Every float comparison is on the uint32 view.  The derived error bounds are half a quantisation step
with 1 % for the f32 roundings (the steps are stated beside each bound).
"""
import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import scene
import export_restate as er
import pack_restate as pr
from support import F, ROOT, TAPS, cached, code_of, frame_taps, guarded, host_sources, is_fill, mk, raw_export, special_records

_mk = functools.partial(mk, exact=True, state=True)
U = np.uint32
HID, SEL = er.HIDDEN, er.SELECTED
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
SYMBOLS = ("gs_pack_encode", "gs_pack_decode", "gs_pack_save", "gs_pack_load", "gs_pack_logit_table", "gs_export_packed", "gs_upload_packed",
           "gs_append_packed")
SIZES = [0, 1, 255, 256, 257, 513, 3001]  # nothing, a lone splat, a chunk less one, one chunk, one plus one, two plus one, the ragged fixture
NEW = 0xA6


def f32(*words):
    return np.array(words, U).view(F)


def cases(n):
    """n special records (NaN, payload NaN, -0, +-inf, a denormal in carried floats) with what the codec branches on added: logits
    beyond +-89, at the exp's limits, infinite and NaN; zero, denormal, underflowing, overflowing, negative-dominant, tied and NaN
    quaternions; log-scales beyond +-20; positions that span more than f32 holds; SH coefficients at and beyond the byte's range."""
    def make():
        if n == 0:
            return np.zeros((0, 80), F)
        rec = np.array(special_records(n), dtype=F, copy=True)
        edits = [(12, [100.0]), (12, [-100.0]), (12, [89.5]), (12, [-104.5]), (12, [np.inf]), (12, [-np.inf]), (12, [np.nan]), (12, [-0.0]),
                 (8, [0.0, 0.0, 0.0, 0.0]), (8, [1e-45, 0.0, 0.0, 0.0]), (8, [1e-30, 0.0, 0.0, 0.0]), (8, [3e38, 3e38, 0.0, 0.0]),
                 (8, [-2.0, 0.1, 0.0, 0.0]), (8, [0.5, 0.5, 0.5, 0.5]), (8, [0.5, -0.5, 0.5, -0.5]), (8, [0.0, -1.0, 0.0, 0.0]),
                 (8, [np.nan, 1.0, 0.0, 0.0]), (8, [0.0, 0.0, 0.3, -0.3]), (4, [25.0, -30.0, 20.0]), (4, [-20.0, np.inf, -np.inf]),
                 (0, [3e38, -3e38, 1.0]), (0, [-3e38, 3e38, -1.0]), (16, [1e38, -1e38, 0.0]),
                 (20, [3.9, -4.1, 5.0]), (24, [np.nan, np.inf, -np.inf]), (76, [4.0, -4.0, 3.984375])]
        for i, (slot, vals) in enumerate(edits):
            rec[(3 + 11 * i) % n, slot:slot + len(vals)] = np.array(vals, F)
        return rec
    return cached(("packed_cases", n), make)


def plane_of(n):
    i = np.arange(n)
    return (np.where(i % 7 == 3, HID, 0) | np.where(i % 3 == 1, SEL, 0) | ((i * 37) & 0x7C)).astype(np.uint8)  # bit 7 is never set


def table():
    from gsplat import packed
    return cached("packed_logit_table", packed.logit_table)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_packed_abi():
    """The eight symbols are exported without a GPU, declared and listed; the ABI version stays 3; null arguments are refused with a
    message that names the call and write nothing."""
    from gsplat import _abi
    L = _abi.load()
    hdr = host_sources().hdr
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
        assert "int32_t %s(" % name in hdr
    assert L.gs_abi_version() == 3 and "#define GS_ABI_VERSION 3\n" in hdr
    assert hdr.index("---- clusters") < hdr.index("---- packed scenes") < hdr.index("---- stand-alone stages")
    assert ctypes.sizeof(_abi.GsPackInfo) == 32 and _abi.GsPackInfo.nonfinite.offset == 24
    assert (_abi.GS_PACK_ORDER_INDEX, _abi.GS_PACK_ORDER_MORTON) == (0, 1)
    assert "#define GS_PACK_ORDER_INDEX 0" in hdr and "#define GS_PACK_ORDER_MORTON 1" in hdr
    info = _abi.GsPackInfo(7, 7, 7, 7)
    first, m = ctypes.c_uint64(77), ctypes.c_uint64(78)
    rec, deg = ctypes.c_void_p(5), ctypes.c_int32(9)
    one = np.zeros((1, 80), F)
    refused = [(lambda: L.gs_export_packed(None, b"x.ply", 0, 0, 3, 1, ctypes.byref(info), None), b"gs_export_packed"),
               (lambda: L.gs_upload_packed(None, b"x.ply", ctypes.byref(first)), b"gs_upload_packed"),
               (lambda: L.gs_append_packed(None, b"x.ply", 0, ctypes.byref(first), ctypes.byref(m)), b"gs_append_packed"),
               (lambda: L.gs_append_packed(None, None, 0, ctypes.byref(first), ctypes.byref(m)), b"gs_append_packed"),
               (lambda: L.gs_pack_load(None, ctypes.byref(rec), ctypes.byref(first), ctypes.byref(deg)), b"gs_pack_load"),
               (lambda: L.gs_pack_load(b"x.ply", None, ctypes.byref(first), ctypes.byref(deg)), b"gs_pack_load"),
               (lambda: L.gs_pack_save(None, one.ctypes.data, 1, 3), b"gs_pack_save"),
               (lambda: L.gs_pack_save(b"x.ply", None, 1, 3), b"gs_pack_save"),
               (lambda: L.gs_pack_encode(None, 1, 3, None, None, None, None), b"gs_pack_encode"),
               (lambda: L.gs_pack_decode(None, None, None, 1, 3, None), b"gs_pack_decode"),
               (lambda: L.gs_pack_logit_table(None), b"gs_pack_logit_table")]
    for call, who in refused:
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        assert who + b":" in L.gs_last_error() and b"null" in L.gs_last_error(), L.gs_last_error()
    assert L.gs_append_packed(None, b"x.ply", 0x100, ctypes.byref(first), ctypes.byref(m)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_append_packed:" in L.gs_last_error() and b"new_state" in L.gs_last_error()
    for call, who in ((lambda: L.gs_pack_encode(one.ctypes.data, 0, 4, None, None, None, None), b"gs_pack_encode"),
                      (lambda: L.gs_pack_save(b"x.ply", one.ctypes.data, 1, -1), b"gs_pack_save")):
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        assert who + b":" in L.gs_last_error() and b"sh_degree" in L.gs_last_error()
    assert (first.value, m.value, rec.value, deg.value) == (77, 78, 5, 9)
    assert (info.count, info.chunks, info.file_bytes, info.nonfinite) == (7, 7, 7, 7)
    assert not os.path.exists("x.ply")


def test_packed_module_surface():
    """gsplat.packed is a module of free functions with the stated signatures; the host classes are untouched (test_abi pins them)."""
    import gsplat
    from gsplat import packed
    assert gsplat.packed is packed
    want = {"save": "(r, path, mask=0, value=0, sh_degree=3, order='morton', with_ids=False)", "upload": "(r, path)",
            "append": "(r, path, state=0)", "encode": "(records, sh_degree=3)", "decode": "(chunks, vertices, sh, sh_degree=3)",
            "save_records": "(path, records, sh_degree=3)", "load_records": "(path)", "logit_table": "()", "rest_count": "(sh_degree)"}
    live = {n: str(inspect.signature(f)) for n, f in vars(packed).items()
            if inspect.isfunction(f) and f.__module__ == packed.__name__ and not n.startswith("_")}
    assert live == want
    for n in want:
        assert getattr(packed, n).__doc__


@pytest.mark.parametrize("n", SIZES)
def test_host_codec_matches_the_restatement(n):
    """gs_pack_encode at degrees 0..3 on the special records: chunk records, vertices, SH bytes and the count of replaced floats
    equal the restatement; gs_pack_decode of them equals the restated decode under the library's table.  Bit for bit."""
    from gsplat import packed
    rec = cases(n)
    if n >= 255:
        assert not np.isfinite(rec[:, er.CARRIED]).all()
    for degree in range(4):
        chunks, verts, sh, bad = packed.encode(rec, degree)
        wc, wv, ws, wbad = pr.encode(rec, degree)
        np.testing.assert_array_equal(pr.bits(chunks), pr.bits(wc), err_msg="chunks, degree %d" % degree)
        np.testing.assert_array_equal(verts, wv, err_msg="vertices, degree %d" % degree)
        np.testing.assert_array_equal(sh, ws, err_msg="sh, degree %d" % degree)
        assert bad == wbad and (n < 255 or bad > 0)
        assert chunks.shape == ((n + 255) // 256, 18) and sh.shape == (n, 3 * pr.rest_count(degree))
        got = packed.decode(chunks, verts, sh, degree)
        want = pr.decode(wc, wv, ws, degree, table())
        np.testing.assert_array_equal(pr.bits(got), pr.bits(want), err_msg="decode, degree %d" % degree)
        assert np.isfinite(got).all()
        assert not pr.bits(got)[:, er.PADDING].any() and not pr.bits(got)[:, 16 + 4 * (degree + 1) ** 2:].any()
    # a chunk's bounds come from its own entries only: the last, partial chunk alone gives the same record
    if n > 256:
        tail = rec[(n - 1) // 256 * 256:]
        np.testing.assert_array_equal(pr.bits(packed.encode(tail, 0)[0][0]), pr.bits(packed.encode(rec, 0)[0][-1]))


def test_codec_branches_are_reached():
    """The special records reach what the codec branches on: every dominant index L, a negated quaternion, the identity fallback,
    both ends of every code, alpha codes 0 and 255, and a -0 among a chunk's bounds candidates."""
    rec = cases(3001)
    _, verts, sh, _ = pr.encode(rec, 3)
    assert set((verts[:, 1] >> U(30)).tolist()) == {0, 1, 2, 3}
    assert {0, 255} <= set((verts[:, 3] & U(255)).tolist())
    assert {0, 2047} <= set((verts[:, 0] >> U(21)).tolist()) and {0, 255} <= set(sh.ravel().tolist())
    ident = pr.rotation_word(np.zeros((1, 4), F))[0]
    assert ident == ((512 << 20) | (512 << 10) | 512) and (verts[:, 1] == ident).sum() >= 4
    q = rec[:, 8:12]
    assert (q[np.arange(3001), np.argmax(np.abs(np.nan_to_num(q)), axis=1)] < 0).any()


def test_logit_table():
    """gs_pack_logit_table: finite, strictly increasing, every entry within 1 f32 ulp of numpy's float64 evaluation."""
    t = table()
    assert t.dtype == F and t.shape == (256,) and np.isfinite(t).all() and (np.diff(t) > 0).all()
    want = pr.logit_table64()
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    assert (np.abs(t.astype(np.float64) - want) <= ulp).all()
    assert t[0] < -6.0 and t[255] > 6.0 and abs(float(t[128]) + float(t[127])) < 1e-6


@pytest.mark.parametrize("n,degree", [(0, 0), (0, 3), (1, 3), (257, 0), (257, 1), (513, 2), (3001, 3)])
def test_file_round_trip(tmp_path, n, degree):
    """gs_pack_save writes exactly the restated file (the header text, the three sections, the implied size); gs_pack_load gives
    the restated decode of it."""
    from gsplat import packed
    rec = cases(n)
    path = tmp_path / "a.packed.ply"
    packed.save_records(path, rec, degree)
    raw = path.read_bytes()
    assert raw == pr.file_bytes(rec, degree)
    assert raw.startswith(pr.header(n, degree)) and len(raw) == len(pr.header(n, degree)) + (n + 255) // 256 * 72 + n * 16 + n * 3 * pr.rest_count(degree)
    assert (b"element sh" in raw) == (degree > 0)
    m, d, chunks, verts, sh = pr.split_file(raw)
    got, deg = packed.load_records(path)
    assert (m, d, deg, got.shape) == (n, degree, degree, (n, 80))
    np.testing.assert_array_equal(pr.bits(got), pr.bits(pr.decode(chunks, verts, sh, degree, table())))


def test_header_text():
    """The header is exactly the one gs_abi.h states, line for line."""
    h = pr.header(300, 1).decode().split("\n")
    assert h[:4] == ["ply", "format binary_little_endian 1.0", "comment gsplat-packed 1", "element chunk 2"]
    assert h[4:22] == ["property float " + p for p in pr.CHUNK_PROPS] and len(pr.CHUNK_PROPS) == 18
    assert h[22:27] == ["element vertex 300"] + ["property uint " + p for p in pr.VERTEX_PROPS]
    assert h[27:] == ["element sh 300"] + ["property uchar f_rest_%d" % k for k in range(9)] + ["end_header", ""]
    assert pr.header(0, 0).decode().split("\n")[22:] == ["element vertex 0"] + ["property uint " + p for p in pr.VERTEX_PROPS] + ["end_header", ""]


def test_derived_error_bounds():
    """Finite random records through the library's codec: position and log-scale within 0.505 (hi - lo) / T of the clamped
    original per axis and chunk (T = 2047, 1023, 2047), the three stored rotation components within 0.505 sqrt(2) / 1023, SH rest
    within 0.505 * 8 / 256 where |v| < 3.9."""
    from gsplat import packed
    rng = np.random.default_rng(2024)
    n = 3001
    rec = np.zeros((n, 80), F)
    rec[:, 0:3] = rng.normal(0, 3, (n, 3))
    rec[:, 4:7] = rng.uniform(-25, 25, (n, 3))
    rec[:, 8:12] = rng.normal(0, 1, (n, 4))
    rec[:, 12] = rng.normal(0, 4, n)
    rec[:, er.CARRIED[11:]] = rng.uniform(-3.9, 3.9, (n, 48)).astype(F)
    chunks, verts, sh, bad = packed.encode(rec, 3)
    assert bad == 0
    got = packed.decode(chunks, verts, sh, 3).astype(np.float64)
    b = chunks.astype(np.float64)[np.arange(n) // 256]
    T = np.array([2047.0, 1023.0, 2047.0])
    worst = {}
    for name, cols, lo, hi, orig in (("position", slice(0, 3), b[:, 0:3], b[:, 3:6], rec[:, 0:3].astype(np.float64)),
                                     ("scale", slice(4, 7), b[:, 6:9], b[:, 9:12], np.clip(rec[:, 4:7].astype(np.float64), -20, 20))):
        step = (hi - lo) / T
        err = np.abs(got[:, cols] - orig)
        assert (err <= 0.505 * step).all(), name
        worst[name] = float((err / step).max())
    q = rec[:, 8:12].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    L = (verts[:, 1] >> U(30)).astype(np.int64)
    np.testing.assert_array_equal(L, np.argmax(np.abs(q.astype(F)), axis=1))
    q *= np.where(q[np.arange(n), L] < 0, -1.0, 1.0)[:, None]
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[L]
    rows = np.arange(n)[:, None]
    err = np.abs(got[:, 8:12][rows, others] - q[rows, others])
    assert (err <= 0.505 * np.sqrt(2.0) / 1023.0).all()
    worst["rotation"] = float(err.max() / (np.sqrt(2.0) / 1023.0))
    rest = er.CARRIED[14:]
    err = np.abs(got[:, rest] - rec[:, rest].astype(np.float64))
    assert (err <= 0.505 * 8.0 / 256.0).all()
    worst["sh"] = float(err.max() / (8.0 / 256.0))
    print("worst error in quantisation steps:", worst)
    assert all(v > 0.45 for v in worst.values())  # the bounds are about the codec, not about a sample that avoids the margins


def test_loader_refusals(tmp_path):
    """A file without the marker, with a renamed or retyped property, a chunk count that does not fit, one byte short, one byte
    long, or an sh element at degree 0 is refused with a message naming the path and the defect; the outputs stay as they were."""
    from gsplat import _abi, packed
    L = _abi.load()
    good = pr.file_bytes(cases(300), 2)
    hdr = pr.header(300, 2)

    def swapped(a, b):
        assert good.count(a) == 1
        return good.replace(a, b)
    empty_sh = pr.header(0, 0).replace(b"end_header\n", b"element sh 0\nend_header\n")
    bad = [(swapped(b"comment gsplat-packed 1\n", b""), "marker"), (swapped(b"uint packed_scale", b"uint packed_size"), "vertex property"),
           (swapped(b"property float min_r", b"property double min_r"), "chunk property"), (swapped(b"f_rest_7\n", b"f_rest_70\n"), "sh property"),
           (swapped(b"element chunk 2", b"element chunk 3"), "chunk count"), (swapped(b"element sh 300", b"element sh 299"), "sh count"),
           (swapped(b"element vertex 300", b"element vertex 4000000000"), "element vertex"), (good[:-1], "bytes"), (good + b"\0", "bytes"),
           (hdr, "bytes"), (good[:len(hdr) - 5], "header"), (empty_sh, "degree 1, 2 or 3"), (b"", "ply")]
    path = tmp_path / "bad.packed.ply"
    for raw, words in bad:
        path.write_bytes(raw)
        rec, n, deg = ctypes.c_void_p(5), ctypes.c_uint64(77), ctypes.c_int32(9)
        assert L.gs_pack_load(str(path).encode(), ctypes.byref(rec), ctypes.byref(n), ctypes.byref(deg)) == _abi.GS_ERR_INVALID_ARGUMENT, words
        msg = L.gs_last_error().decode()
        assert "gs_pack_load" in msg and str(path) in msg and words in msg, msg
        assert (rec.value, n.value, deg.value) == (5, 77, 9)
    path.write_bytes(good)
    assert packed.load_records(path)[0].shape == (300, 80)
    code, msg = code_of(lambda: packed.load_records(tmp_path / "none.ply"))
    assert code == _abi.GS_ERR_INVALID_ARGUMENT and "cannot open" in msg


def test_morton_restatement():
    """The restated order is a permutation, stable on duplicate positions, the index order when all positions coincide, and puts
    non-finite positions last (in index order); the keys interleave x, y, z from bit 0."""
    rng = np.random.default_rng(5)
    pos = rng.normal(0, 2, (1000, 3)).astype(F)
    pos[100:110] = pos[50]
    pos[[7, 500, 999], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    order = pr.morton_order(pos)
    assert sorted(order.tolist()) == list(range(1000))
    assert order[-3:].tolist() == [7, 500, 999]
    dup = [int(np.flatnonzero(order == i)[0]) for i in [50] + list(range(100, 110))]
    assert dup == list(range(dup[0], dup[0] + 11))
    keys = pr.morton_keys(pos)
    assert (keys[[7, 500, 999]] == pr.KEY_LAST).all() and (np.delete(keys, [7, 500, 999]) < pr.KEY_LAST).all()
    assert (np.diff(keys[order].astype(np.int64)) >= 0).all()
    same = np.tile(f32(0x40490FDB, 0x80000000, 0x00000001), (300, 1))
    assert pr.morton_order(same).tolist() == list(range(300)) and (pr.morton_keys(same) == 0).all()
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], F)
    assert pr.morton_keys(corners).tolist() == [0, 0x09249249, 0x09249249 << 1, 0x09249249 << 2, 0x3FFFFFFF]
    assert pr.morton_order(np.zeros((0, 3), F)).size == 0


def _sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "pack_check", "main.cpp"), "-x", "c++", os.path.join(CSRC, "gs_pack_host.hip"),
                           "-o", exe])
    return exe


def test_sanitized_host_program(tmp_path):
    """tools/pack_check: the host codec and the file parser compiled alone with -fsanitize=address,undefined and run over every
    chunk margin, file round trips, truncated and garbled headers and the format's refusals; and the host twin of the canonical
    exp, which that program prints, equals oracle/np_oracle.expf bit for bit.  Skipped where the sanitizer runtime is not installed."""
    from oracle import np_oracle as npo
    exe = _sanitized(tmp_path)
    work = tmp_path / "work"
    work.mkdir()
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "pack_check ok" in out.stdout
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-104.5, 89.5, 1500), rng.normal(0, 1, 400), [0.0, -0.0, 88.72283935546875, 88.7228469848633, -103.97208404541016,
                        -103.97209167480469, 100.0, -110.0, np.inf, -np.inf, 1e-45, -1e-45, 0.693145751953125, -87.5, 87.5]]).astype(F)
    res = subprocess.run([exe, "--exp"] + ["%08x" % w for w in x.view(U)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.array([int(w, 16) for w in res.stdout.split()], U)
    np.testing.assert_array_equal(got, npo.expf(x).view(U))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
FILTERS = [(0, 0), (HID, 0), (SEL, SEL)]


def _export(r, path, filt, degree, order):
    """gs_export_packed with a guarded id buffer: (info dict, ids, the file's bytes)."""
    from gsplat import _abi
    L = _abi.load()
    n = r.numGaussians
    ids = guarded(n + 1, U)
    info = _abi.GsPackInfo()
    _abi.check(L.gs_export_packed(r._ctx, str(path).encode(), filt[0], filt[1], degree, order, ctypes.byref(info), ids.ctypes.data))
    assert is_fill(ids[info.count:])
    return info, ids[:info.count].copy(), open(path, "rb").read()


def _same_file(raw, rec, degree, info, bad):
    """The file is the restatement's of these records in this order: header, chunk records, vertices, SH bytes, and the info."""
    n = rec.shape[0]
    m, d, chunks, verts, sh = pr.split_file(raw)
    wc, wv, ws, wbad = pr.encode(rec, degree)
    assert (m, d) == (n, degree)
    np.testing.assert_array_equal(pr.bits(chunks), pr.bits(wc), err_msg="chunk records")
    np.testing.assert_array_equal(verts, wv, err_msg="vertices")
    np.testing.assert_array_equal(sh, ws, err_msg="sh bytes")
    assert raw == pr.file_bytes(rec, degree)
    assert (info.count, info.chunks, info.file_bytes, info.nonfinite) == (n, (n + 255) // 256, len(raw), wbad)
    assert bad is None or (wbad > 0) == bad


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES[1:])
def test_export_packed_index_order(tmp_path, n):
    """gs_export_packed in index order on the special records, every filter: the file's three sections, info and ids equal the
    restatement applied to gs_export_splats of the same filter, bit for bit; a filter that matches nothing writes a valid empty file."""
    from gsplat import _abi, packed
    rec = cases(n)
    r = _mk(rec, 64, 64, 8)
    r.write_state(plane_of(n))
    path = tmp_path / "out.packed.ply"
    for filt in FILTERS:
        want, want_ids = raw_export(r, filt[0], filt[1], True)
        for degree in (0, 3) + ((1, 2) if n == 257 else ()):
            info, ids, raw = _export(r, path, filt, degree, _abi.GS_PACK_ORDER_INDEX)
            np.testing.assert_array_equal(ids, want_ids)
            _same_file(raw, want, degree, info, None)
    for degree in (0, 3):
        info, ids, raw = _export(r, path, (0x80, 0x80), degree, _abi.GS_PACK_ORDER_INDEX)
        assert raw == pr.header(0, degree) and ids.size == 0 and (info.count, info.chunks, info.nonfinite) == (0, 0, 0)
        assert packed.load_records(path)[0].shape == (0, 80)
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", [(3001, "mixed"), (257, "mixed"), (257, "identical")])
def test_export_packed_morton_order(tmp_path, n, kind):
    """gs_export_packed along the Morton curve: ids equals the restated order of the filter's splats (duplicate positions stay in
    index order, identical positions give the index order, non-finite positions come last) and the sections are the restatement's of
    the records in that order."""
    from gsplat import _abi
    rec = np.array(cases(n), copy=True)
    if kind == "identical":
        rec[:, 0:3] = f32(0x3F9E0652, 0x80000000, 0xC0200000)
    else:
        rec[40:52, 0:3] = rec[33, 0:3]
        rec[n - 1, 0:3] = rec[0, 0:3]
        assert not np.isfinite(rec[:, 0:3]).all()
    r = _mk(rec, 64, 64, 8)
    r.write_state(plane_of(n))
    path = tmp_path / "out.packed.ply"
    for filt, degree in (((0, 0), 3), ((SEL, SEL), 0), ((HID, 0), 1)):
        want, want_ids = raw_export(r, filt[0], filt[1], True)
        order = pr.morton_order(want[:, 0:3])
        info, ids, raw = _export(r, path, filt, degree, _abi.GS_PACK_ORDER_MORTON)
        np.testing.assert_array_equal(ids, want_ids[order])
        if kind == "identical":
            np.testing.assert_array_equal(ids, want_ids)
        _same_file(raw, want[order], degree, info, None)
    r.destroy()


def _plain(n):
    from gsplat import synth
    return cached(("packed_plain", n), lambda: np.ascontiguousarray((synth.bicycle_like(3001) if n == 3001 else scene(10000))[:n]))


def _uniforms():
    from gpu_checks import orbit_uniforms
    return orbit_uniforms(64, 64)


def _same_taps(r, fresh, u):
    for debug in (False, True):
        a, b = frame_taps(r, u, debug), frame_taps(fresh, u, debug)
        for t in TAPS + ("rgba8", "rgbf"):
            np.testing.assert_array_equal(a[t].view(U) if a[t].dtype == F else a[t], b[t].view(U) if b[t].dtype == F else b[t],
                                          err_msg="%s debug=%s" % (t, debug))


@pytest.mark.gpu
@pytest.mark.parametrize("n,degree", [(1, 3), (257, 1), (3001, 3)])
def test_upload_packed(tmp_path, n, degree):
    """gs_upload_packed: the context's records equal the restated decode of the file bit for bit (special records, no frame), and
    on a scene that renders an EXACT frame's taps equal those of a fresh context given gs_upload_splats of the decoded records."""
    from gsplat import packed
    path = tmp_path / "in.packed.ply"
    for rec, render in ((cases(n), False), (_plain(n), True)):
        packed.save_records(path, rec, degree)
        m, d, chunks, verts, sh = pr.split_file(path.read_bytes())
        want = pr.decode(chunks, verts, sh, degree, table())
        r = _mk(_plain(5), 64, 64, 8)
        assert packed.upload(r, path) == n == r.numGaussians == r.stats()["num_gaussians"]
        got, ids = raw_export(r, 0, 0, True)
        np.testing.assert_array_equal(pr.bits(got), pr.bits(want))
        np.testing.assert_array_equal(ids, np.arange(n, dtype=U))
        assert not r.read_state().any()
        if render:
            fresh = _mk(want, 64, 64, 8)
            _same_taps(r, fresh, _uniforms())
            fresh.destroy()
        r.destroy()


@pytest.mark.gpu
def test_more_than_one_trip(tmp_path):
    """70 001 splats: more than one trip of the export's bounce buffers (1 MiB: 65 536 vertices) and of the loader's staging (65 536
    vertices, 256 whole chunks), a last trip that ends in a partial chunk, and a Morton sort of more than one tile.  The file equals
    the restatement's in both orders; the uploaded scene equals the restated decode."""
    from gsplat import _abi, packed, synth
    n = 70001
    rec = cached(("packed_plain", n), lambda: synth.bicycle_like(n))
    r = _mk(rec, 64, 64, 8, state=False)
    path = tmp_path / "big.packed.ply"
    want = er.zero_padding(rec)
    info, ids, raw = _export(r, path, (0, 0), 3, _abi.GS_PACK_ORDER_INDEX)
    np.testing.assert_array_equal(ids, np.arange(n, dtype=U))
    _same_file(raw, want, 3, info, False)
    order = pr.morton_order(want[:, 0:3])
    info, ids, raw = _export(r, path, (0, 0), 1, _abi.GS_PACK_ORDER_MORTON)
    np.testing.assert_array_equal(ids, order.astype(U))
    _same_file(raw, want[order], 1, info, False)
    m, d, chunks, verts, sh = pr.split_file(raw)
    assert packed.upload(r, path) == n
    np.testing.assert_array_equal(pr.bits(raw_export(r, 0, 0, False)[0]), pr.bits(pr.decode(chunks, verts, sh, 1, table())))
    r.destroy()


THREE = 2 * 65536 + 257  # three trips of every 65 536-vertex stream: the first buffer is used again; the last is a whole chunk and one splat


def _three_trips():
    from gsplat import synth
    return cached(("packed_plain", THREE), lambda: synth.bicycle_like(THREE))


@pytest.mark.gpu
def test_three_trips(tmp_path):
    """131 329 splats: the vertex section is three trips of the export's 1 MiB ring and the SH section at degree 3 six, so both pinned
    buffers are written again after the host has consumed them; the loader's staging makes three trips, the last of one whole chunk
    and one splat.  Both files equal the restatement's byte for byte, ids included; the uploaded scene equals the restated decode."""
    from gsplat import _abi, packed
    n = THREE
    rec = _three_trips()
    assert (n * 16 + (1 << 20) - 1) >> 20 == 3 and (n * 45 + (1 << 20) - 1) >> 20 == 6 and n % 65536 == 257
    r = _mk(rec, 64, 64, 8, state=False)
    path = tmp_path / "three.packed.ply"
    want = er.zero_padding(rec)
    info, ids, raw = _export(r, path, (0, 0), 3, _abi.GS_PACK_ORDER_INDEX)
    np.testing.assert_array_equal(ids, np.arange(n, dtype=U))
    _same_file(raw, want, 3, info, False)
    order = pr.morton_order(want[:, 0:3])
    info, ids, raw = _export(r, path, (0, 0), 1, _abi.GS_PACK_ORDER_MORTON)
    np.testing.assert_array_equal(ids, order.astype(U))
    _same_file(raw, want[order], 1, info, False)
    m, d, chunks, verts, sh = pr.split_file(raw)
    assert packed.upload(r, path) == n
    np.testing.assert_array_equal(pr.bits(raw_export(r, 0, 0, False)[0]), pr.bits(pr.decode(chunks, verts, sh, 1, table())))
    r.destroy()


@pytest.mark.gpu
def test_append_packed_three_trips(tmp_path):
    """A packed file of 131 329 splats (degree 3: the largest trips) behind 300 resident ones: the context equals one built by
    insert.append of the decoded records -- records, ids, first, state bytes and splat count."""
    from gsplat import insert, packed
    n = THREE
    head = np.ascontiguousarray(_plain(300))
    path = tmp_path / "tail.packed.ply"
    packed.save_records(path, _three_trips(), 3)
    m, d, chunks, verts, sh = pr.split_file(path.read_bytes())
    decoded = pr.decode(chunks, verts, sh, 3, table())
    r, fresh = _mk(head, 64, 64, 8), _mk(head, 64, 64, 8)
    for x in (r, fresh):
        x.write_state(plane_of(300))
    assert packed.append(r, path, NEW) == (300, n) == insert.append(fresh, decoded, NEW)
    assert r.numGaussians == 300 + n == r.stats()["num_gaussians"] == fresh.stats()["num_gaussians"]
    (a, ai), (b, bi) = raw_export(r, 0, 0, True), raw_export(fresh, 0, 0, True)
    np.testing.assert_array_equal(pr.bits(a), pr.bits(b))
    np.testing.assert_array_equal(pr.bits(a[300:]), pr.bits(decoded))
    np.testing.assert_array_equal(ai, bi)
    np.testing.assert_array_equal(ai, np.arange(300 + n, dtype=U))
    np.testing.assert_array_equal(r.read_state(), np.concatenate([plane_of(300), np.full(n, NEW, np.uint8)]))
    np.testing.assert_array_equal(r.read_state(), fresh.read_state())
    fresh.destroy()
    r.destroy()


@pytest.mark.gpu
def test_append_packed(tmp_path):
    """257 packed splats behind 300 resident ones: the context equals one built by insert.append of the decoded records (records,
    ids, first, state bytes, taps); a borrowing context and a refused file leave the scene and its next frame unchanged."""
    from gsplat import _abi, insert, packed
    base = _plain(557)
    head, tail = np.ascontiguousarray(base[:300]), np.ascontiguousarray(base[300:])
    path = tmp_path / "tail.packed.ply"
    packed.save_records(path, tail, 2)
    m, d, chunks, verts, sh = pr.split_file(path.read_bytes())
    decoded = pr.decode(chunks, verts, sh, 2, table())
    u = _uniforms()
    r, fresh = _mk(head, 64, 64, 8), _mk(head, 64, 64, 8)
    for x in (r, fresh):
        x.write_state(plane_of(300))
        frame_taps(x, u, False)
    assert packed.append(r, path, NEW) == (300, 257) == insert.append(fresh, decoded, NEW)
    assert r.numGaussians == 557 == r.stats()["num_gaussians"]
    (a, ai), (b, bi) = raw_export(r, 0, 0, True), raw_export(fresh, 0, 0, True)
    np.testing.assert_array_equal(pr.bits(a), pr.bits(b))
    np.testing.assert_array_equal(pr.bits(a[300:]), pr.bits(decoded))
    np.testing.assert_array_equal(ai, bi)
    np.testing.assert_array_equal(r.read_state(), np.concatenate([plane_of(300), np.full(257, NEW, np.uint8)]))
    np.testing.assert_array_equal(r.read_state(), fresh.read_state())
    _same_taps(r, fresh, u)
    fresh.destroy()
    # refusals: the scene and its next frame stay
    before, state_before = raw_export(r, 0, 0, False)[0], r.read_state()
    img = frame_taps(r, u, False)["rgba8"]
    bad = tmp_path / "bad.packed.ply"
    bad.write_bytes(path.read_bytes()[:-1])

    def unchanged():
        np.testing.assert_array_equal(pr.bits(raw_export(r, 0, 0, False)[0]), pr.bits(before))
        np.testing.assert_array_equal(r.read_state(), state_before)
        np.testing.assert_array_equal(frame_taps(r, u, False)["rgba8"], img)
        assert r.numGaussians == 557 == r.stats()["num_gaussians"]
    for fn, words in ((lambda: packed.append(r, bad, NEW), "bytes"), (lambda: packed.append(r, tmp_path / "none.ply", NEW), "cannot open"),
                      (lambda: packed.append(r, path, 0x100), "new_state")):
        code, msg = code_of(fn)
        assert code == _abi.GS_ERR_INVALID_ARGUMENT and words in msg and "gs_append_packed" in msg, msg
        unchanged()
    b = _mk(head, 64, 64, 8, share_with=r)
    code, msg = code_of(lambda: packed.append(b, path, 0))
    assert code == _abi.GS_ERR_INVALID_ARGUMENT and "owner" in msg
    b.destroy()
    unchanged()
    r.destroy()


@pytest.mark.gpu
def test_export_changes_nothing(tmp_path):
    """A frame's taps before and after gs_export_packed (both orders) are equal, with frames in flight at the default depth; a
    context without GS_FLAG_SPLAT_STATE exports every splat and refuses a non-zero filter as the other edits do; bad arguments are
    refused and leave no file."""
    from gsplat import _abi, packed
    rec = _plain(3001)
    u = _uniforms()
    r = _mk(rec, 64, 64, 8)
    r.write_state(plane_of(3001))
    before = [frame_taps(r, u, debug) for debug in (False, True)]
    state = r.read_state()
    path = tmp_path / "out.packed.ply"
    r.render_uniforms(u)  # in flight while the export begins: the call drains the ring first
    for order in ("morton", "index"):
        info = packed.save(r, path, SEL, SEL, 3, order)
        assert info["count"] == int((state & SEL != 0).sum()) and info["file_bytes"] == os.path.getsize(path) and info["nonfinite"] == 0
    after = [frame_taps(r, u, debug) for debug in (False, True)]
    for a, b in zip(before, after):
        for t in TAPS + ("rgba8", "rgbf"):
            np.testing.assert_array_equal(a[t], b[t], err_msg=t)
    np.testing.assert_array_equal(r.read_state(), state)
    np.testing.assert_array_equal(pr.bits(raw_export(r, 0, 0, False)[0]), pr.bits(er.zero_padding(rec)))
    # the round trip through a file renders: upload what was saved
    info, ids = packed.save(r, path, 0, 0, 3, "morton", with_ids=True)
    assert sorted(ids.tolist()) == list(range(3001)) and info["count"] == 3001
    assert packed.upload(r, path) == 3001
    frame_taps(r, u, False)
    L = _abi.load()
    os.remove(path)
    for call, words in ((lambda: L.gs_export_packed(r._ctx, str(path).encode(), 0, 0, 4, 0, None, None), b"sh_degree"),
                        (lambda: L.gs_export_packed(r._ctx, str(path).encode(), 0, 0, 3, 2, None, None), b"order"),
                        (lambda: L.gs_export_packed(r._ctx, None, 0, 0, 3, 0, None, None), b"null path"),
                        (lambda: L.gs_export_packed(r._ctx, str(path).encode(), 0x100, 0, 3, 0, None, None), b"state byte"),
                        (lambda: L.gs_export_packed(r._ctx, str(tmp_path / "no" / "dir.ply").encode(), 0, 0, 3, 0, None, None), b"cannot create")):
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        assert b"gs_export_packed" in L.gs_last_error() and words in L.gs_last_error(), L.gs_last_error()
        assert not os.path.exists(path)
    r.destroy()
    plain = _mk(rec, 64, 64, 8, state=False)
    assert packed.save(plain, path, order="index")["count"] == 3001
    assert path.read_bytes() == pr.file_bytes(er.zero_padding(rec), 3)
    code, msg = code_of(lambda: packed.save(plain, path, SEL, SEL))
    assert code == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
    plain.destroy()
