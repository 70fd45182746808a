"""CPU: clip_delta_e's host side -- the record layout and the exported symbol, the refusals that need no GPU, DeltaEReport's arithmetic on hand-made
histograms, and the host build of the kernel's pixel function (csrc/metrics_ops.h) against the oracle on the inputs of the GPU test."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import metrics_util as mu
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import metrics
from vsdeoldify_amd.havc import HAVCError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def test_record_layout_matches_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "havc_mi355.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d\\n",'
                   "sizeof(havc_de_rec),offsetof(havc_de_rec,sum),offsetof(havc_de_rec,max),offsetof(havc_de_rec,sse),offsetof(havc_de_rec,hist),"
                   "offsetof(havc_de_rec,reserved),HAVC_DE_BINS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = nat.DE_REC_DTYPE
    assert got == [d.itemsize, d.fields["sum"][1], d.fields["max"][1], d.fields["sse"][1], d.fields["hist"][1], d.fields["reserved"][1], nat.DE_BINS]
    assert d.itemsize == 4144 and d["hist"].shape == (1025,) and d["sse"].shape == (3,) and nat.DE_BINS == metrics.BINS == mu.BINS


def test_symbol_is_declared_exported_and_bound():
    text = open(HEADER).read()
    m = re.search(r"int havc_delta_e_clip\(havc_ctx\* ctx, const uint8_t\* a, const uint8_t\* b, int width, int height, int n_frames, havc_de_rec\* recs, "
                  r"double\* map\);", text)
    assert m, "havc_delta_e_clip is declared with the issue's signature"
    syms = {name: (res, args) for name, res, args in nat.SYMBOLS}
    assert len(syms["havc_delta_e_clip"][1]) == 8 and len(syms["havc_delta_e_set_table"][1]) == 2
    lib = nat.load()
    assert lib.havc_delta_e_clip and lib.havc_delta_e_set_table
    import vsdeoldify_amd
    assert vsdeoldify_amd.clip_delta_e is metrics.clip_delta_e and vsdeoldify_amd.DeltaEReport is metrics.DeltaEReport


def test_refusals_need_no_context(monkeypatch):
    from vsdeoldify_amd import render
    monkeypatch.setattr(render, "get_context", lambda *a, **k: pytest.fail("a refusal reached the GPU"))
    ok = np.zeros((2, 4, 5, 3), np.uint8)
    for a, b, what in ((None, ok, "not a clip"), (ok, [[1, 2, 3]], "not a clip"), (ok, ok[:, :3], "differ in shape"), (ok, ok[0], "differ in shape"),
                       (ok.astype(np.float32), ok.astype(np.float32), "RGB24"), (ok[..., :2], ok[..., :2], "RGB24"), (ok[0, 0], ok[0, 0], "RGB24"),
                       (ok.astype(np.uint16), ok.astype(np.uint16), "RGB24"), (ok[:0], ok[:0], "zero frames"), (ok[:, :0], ok[:, :0], "zero pixels")):
        with pytest.raises(HAVCError, match=what):
            metrics.clip_delta_e(a, b)


def _report(hists, sums=None, maxes=None, sses=None, n_pixels=None):
    hists = np.asarray(hists, np.uint32)
    recs = np.zeros(len(hists), nat.DE_REC_DTYPE)
    recs["hist"] = hists
    recs["sum"] = 0 if sums is None else sums
    recs["max"] = 0 if maxes is None else maxes
    recs["sse"] = 0 if sses is None else sses
    return metrics.DeltaEReport(recs, int(hists[0].sum()) if n_pixels is None else n_pixels)


def test_report_below_and_percentile_from_hand_made_histograms():
    h = np.zeros(1025, np.uint32)
    h[0], h[63], h[64], h[200] = 50, 30, 15, 5                       # dE in [0, 1/64): 50; [63/64, 1): 30; [1, 65/64): 15; [200/64, 201/64): 5
    r = _report([h])
    assert r.below(1.0) == 0.80 and r.below(1.0, frame=0) == 0.80
    assert r.below(0) == 0.0 and r.below(1 / 64) == 0.50 and r.below(63 / 64) == 0.50 and r.below(65 / 64) == 0.95 and r.below(16.0) == 1.0
    assert r.below(1.0 + 1 / 128) == 0.80                             # between two edges: the bins entirely below
    with pytest.raises(ValueError):
        r.below(16.5)
    with pytest.raises(ValueError):
        r.below(-1)
    # percentile: the upper edge of the bin in which the cumulative count reaches q
    assert r.percentile(50) == 1 / 64                                 # exactly reached at the end of bin 0
    assert r.percentile(50.0001) == 64 / 64                           # the next pixel lies in bin 63
    assert r.percentile(80) == 64 / 64 and r.percentile(80.5) == 65 / 64 and r.percentile(95) == 65 / 64
    assert r.percentile(99) == 201 / 64 and r.percentile(100) == 201 / 64          # the tail above bin 200 is empty
    assert r.percentile(0) == 1 / 64
    with pytest.raises(ValueError):
        r.percentile(101)


def test_report_overflow_bin():
    h = np.zeros(1025, np.uint32)
    h[10], h[1023], h[1024] = 90, 5, 5
    r = _report([h], maxes=[40.0])
    assert r.below(16.0) == 0.95 and r.below(1023 / 64) == 0.90
    assert r.percentile(95) == 16.0 and r.percentile(95.1) == math.inf and r.percentile(100) == math.inf
    assert not r.meets_contract


def test_report_clip_totals_across_frames():
    h0, h1 = np.zeros(1025, np.uint32), np.zeros(1025, np.uint32)
    h0[0], h1[0], h1[70] = 100, 60, 40
    r = _report([h0, h1], sums=[1.0, 50.0], maxes=[0.01, 1.1], sses=[[0, 0, 0], [300, 0, 300]])
    assert r.n_frames == 2 and np.array_equal(r.clip_hist, h0.astype(np.uint64) + h1)
    assert np.array_equal(r.mean, [0.01, 0.5]) and r.clip_mean == 51.0 / 200 and r.clip_max == 1.1
    assert r.below(1.0) == 0.8 and r.below(1.0, frame=0) == 1.0 and r.below(1.0, frame=1) == 0.6
    assert r.percentile(80) == 1 / 64 and r.percentile(81) == 71 / 64 and r.percentile(100, frame=0) == 1 / 64
    assert not r.meets_contract
    r.recs["max"][1] = 0.999
    assert r.meets_contract
    r.recs["max"][1] = 1.0                                            # the contract is strict
    assert not r.meets_contract
    # PSNR over the three channels: frame 1 has MSE 600 / 300 = 2, the clip 600 / 600 = 1; an equal frame gives inf
    assert r.psnr[0] == math.inf and abs(r.psnr[1] - 10 * math.log10(255 ** 2 / 2)) < 1e-12
    assert abs(r.clip_psnr - 10 * math.log10(255 ** 2)) < 1e-12
    assert _report([h0], sses=[[0, 0, 0]]).clip_psnr == math.inf
    assert "NOT met" in r.table() and len(r.table().splitlines()) == 5


def test_table_is_the_oracles_expression():
    c = np.arange(256).astype(np.float64) / 255.0
    t = metrics.srgb_linear_table()
    assert t.dtype == np.float64 and t.tobytes() == np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92).tobytes()


@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("de_host"))
    return mu.build_host(tmp), tmp


def test_structured_inputs_reach_every_branch_and_no_discontinuity():
    """the inputs of the GPU test, on the CPU: every branch of the oracle's np.where's holds pixels, and none lies on the hue discontinuity"""
    a, b, rows = mu.structured_pair()
    counts = mu.branch_counts(a, b)
    assert all(v > 0 for v in counts.values()), counts
    assert int(mu.hue_excluded(a, b).sum()) == 0
    lo, hi = rows["black"]
    v = mu.oracle_intermediates(a[lo:hi], b[lo:hi])
    assert (v["cc"] == 0).all()                                       # black: a = b = 0 exactly, the achromatic branch


def test_host_build_of_the_pixel_function_agrees_with_the_oracle(host_build):
    """csrc/metrics_ops.h compiled for the host with a main of its own, on the structured pair and on random clips of the GPU test's sizes: within LIMIT of
    the oracle (measured here: 4.4e-13), identical pixels exactly 0, bins as floor(dE * 64) capped at 1024"""
    exe, tmp = host_build
    table = metrics.srgb_linear_table()
    a, b, rows = mu.structured_pair()
    got, bins = mu.run_host(exe, tmp, a, b, table)
    err, share = mu.compare_maps(got, a, b)
    print(f"host build vs oracle, structured pair: max |diff| {err:.3e}, excluded share {share}")
    assert share == 0 and err <= mu.LIMIT
    lo, hi = rows["same"]
    assert not got[lo:hi].any() and not got[np.all(a == b, -1)].any()
    assert np.array_equal(bins, np.minimum(np.floor(got * 64), 1024).astype(np.int32)) and bins.max() == 1024
    for shape, seed in (((3, 37, 23, 3), 1), ((1, 255, 257, 3), 2)):
        x, y = mu.random_pair(shape, seed)
        got, _ = mu.run_host(exe, tmp, x, y, table)
        err, _ = mu.compare_maps(got, x, y)
        assert err <= mu.LIMIT, (shape, err)
    # the runtime's default table (the C library's pow) moves a pixel by far less than LIMIT
    got2, _ = mu.run_host(exe, tmp, a[:64], b[:64], None)
    got1, _ = mu.run_host(exe, tmp, a[:64], b[:64], table)
    assert np.abs(got2 - got1).max() <= mu.LIMIT


def test_fixed_order_sum_restatement():
    """the restated reduction on values where the order matters, against a plain loop over the same tree"""
    r = np.random.default_rng(5)
    m = r.random((37, 61)) * 10.0 ** r.integers(-8, 3, (37, 61))
    v = np.zeros(3 * 1024)
    v[:m.size] = m.reshape(-1)
    total = 0.0
    for blk in v.reshape(3, 256, 4):
        t = [((0.0 + float(p[0])) + float(p[1])) + float(p[2]) + float(p[3]) for p in blk]
        s = 128
        while s:
            for i in range(s):
                t[i] = t[i] + t[i + s]
            s //= 2
        total = total + t[0]
    assert mu.fixed_order_sum(m) == total
    assert abs(total - m.sum()) <= 1e-12 * m.sum()
