"""The deterministic forms of the two implicit-GEMM weight-gradient kernels (`ammc_conv_wgrad_s16_det` /
`ammc_conv_wgrad_f32_det`: slabs + a fixed-order sum instead of fp32 atomics) and the `deterministic` switch above them,
without a device: over a grid of descriptors the label's split count is the workspace's, it is what the descriptor alone
says (the formula of the dispatchers written out here), the status codes are those of the atomics entries, the label does
not move with the weight-gradient switch, the older entries did not move, `run_train` knows `--deterministic` and
refuses a resume across the flag, and the engines follow the switch of the module the user calls."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

import wgrad_cases as W
from conftest import ROOT
from ammcnet_aaai2021_amd import _lib
from ammcnet_aaai2021_amd._lib import AmmcWgradDesc

SHAPES = ((1, 9, 7), (2, 16, 15), (2, 24, 20), (2, 15, 21), (3, 32, 32), (4, 64, 64))       # (B, H, W) of g: 2 .. 512 chunks of 32 pixels
NS = (32, 64, 128)
CINS = (8, 16, 64)
S16_KINDS = ((4, 2), (16, 1), (16, 2), (9, 1))            # (ntaps, a_step)
F32_KINDS = ((1, 1), (4, 2), (9, 1), (16, 1), (16, 2))


def desc(B, H, W_, n, cin, ntaps, a_step, g=0x10000000, a=0x20000000, dw=0x30000000, zeros=0x40000000):
    """a dense descriptor over fake addresses (labels and refusals look at values only)"""
    d = AmmcWgradDesc()
    halo = 2 if ntaps == 16 else 1
    ah, aw = (H, W_) if ntaps in (1, 9) else ((2 * H, 2 * W_) if ntaps == 4 else (a_step * H, a_step * W_))
    d.g, d.a, d.dw, d.zeros = g, a, dw, zeros
    d.batch, d.height, d.width, d.n, d.cin, d.ntaps, d.a_step = B, H, W_, n, cin, ntaps, a_step
    d.g_ps, d.g_rs, d.g_bs = n, (W_ + 2) * n, (H + 2) * (W_ + 2) * n
    d.a_ps, d.a_rs, d.a_bs = cin, (aw + 2 * halo) * cin, (ah + 2 * halo) * (aw + 2 * halo) * cin
    return d


def s16_grid():
    for (B, H, W_), n, cin, (ntaps, a_step) in itertools.product(SHAPES, NS, CINS, S16_KINDS):
        if ntaps == 9 and W_ % 32 == 0 and H % 2 == 0:
            # 3x3 stride 1: only what the halo-patch dispatcher turns away (W % 32, odd H) reaches wgrad_s16_kernel through
            # the atomics entry; of the patch-shaped images keep the channel counts it rejects (cin <= 32 under n 32)
            if not (cin <= 32 and n == 32):
                continue
        yield f"s16-{B}x{H}x{W_}-n{n}-cin{cin}-t{ntaps}s{a_step}", desc(B, H, W_, n, cin, ntaps, a_step)


def f32_grid():
    for (B, H, W_), n, cin, (ntaps, a_step) in itertools.product(SHAPES, NS, CINS + (32,), F32_KINDS):
        if ntaps == 1 and cin % 32:
            continue
        yield f"f32-{B}x{H}x{W_}-n{n}-cin{cin}-t{ntaps}s{a_step}", desc(B, H, W_, n, cin, ntaps, a_step)


def kpad(d):
    return (d.ntaps * d.cin + 31) // 32 * 32


def expected_splits(d, form: str) -> int:
    """the pixel splits as the dispatchers compute them: a function of the descriptor alone"""
    if form == "s16":
        br, target = 128, 2 * 256
    else:
        br, target = (128 if d.n % 128 == 0 else (64 if d.n % 64 == 0 else 32)), 4 * 256
    tiles = -(-d.n // br) * -(-kpad(d) // 128)
    nchunks = -(-(d.batch * d.height * d.width) // 32)
    ms = max(1, min(-(-target // tiles), -(-nchunks // 8)))
    per = -(-nchunks // ms)
    return -(-nchunks // per)


def _q(fn, d, n=96):
    buf = C.create_string_buffer(n)
    rc = getattr(_lib.load(), fn)(C.byref(d) if d is not None else None, buf, n)
    return rc, buf.value.decode()


def det_variant(d, form):
    return _q(f"ammc_conv_wgrad_{form}_det_variant", d)


def det_floats(d, form) -> int:
    return int(getattr(_lib.load(), f"ammc_conv_wgrad_{form}_det_floats")(C.byref(d)))


def label_k(label: str) -> int:
    name, k = label.rsplit("+det", 1)
    assert name.startswith("wgrad_"), label
    return int(k)


def test_the_grids_cover_what_the_issue_names():
    s16, f32 = dict(s16_grid()), dict(f32_grid())
    assert len(s16) > 100 and len(f32) > 150
    kinds = {(d.ntaps, d.a_step) for d in s16.values()}
    assert kinds == {(4, 2), (16, 1), (16, 2), (9, 1)}
    assert {d.ntaps for d in f32.values()} == {1, 4, 9, 16}
    for grid in (s16, f32):
        assert {d.n for d in grid.values()} == set(NS) and set(CINS) <= {d.cin for d in grid.values()}
    # every 3x3 descriptor of the S16 grid is one the atomics entry sends to wgrad_s16_kernel, patch-shaped images included
    nine = [d for d in s16.values() if d.ntaps == 9]
    assert any(d.width % 32 == 0 and d.height % 2 == 0 for d in nine) and any(d.width % 32 for d in nine)
    if not any(k in os.environ for k in W.SWITCHES):
        for d in s16.values():
            assert W.variant(d) == (0, W.IM2COL)
    ks = {expected_splits(d, "s16") for d in s16.values()} | {expected_splits(d, "f32") for d in f32.values()}
    assert 1 in ks and 2 in ks and max(ks) >= 64 and any(k >= 3 for k in ks)


@pytest.mark.parametrize("form,grid", [("s16", s16_grid), ("f32", f32_grid)])
def test_label_workspace_and_formula_agree_on_the_split_count(form, grid):
    for name, d in grid():
        rc, label = det_variant(d, form)
        assert rc == 0, (name, rc)
        k = label_k(label)
        assert k == expected_splits(d, form), (name, label)
        floats = det_floats(d, form)
        if k == 1:
            assert floats == 0, (name, floats)              # one split stores straight into dw: no workspace
        else:
            assert floats == k * d.n * kpad(d) and floats // (d.n * kpad(d)) == k, (name, label, floats)
        assert label.startswith("wgrad_s16+det" if form == "s16" else "wgrad_f32<"), label
        assert det_variant(d, form) == (rc, label)          # asked twice


def test_a_label_names_the_f32_instance_of_its_row_count():
    for n, inst in ((32, "wgrad_f32<1, 4, 1, 1>"), (64, "wgrad_f32<1, 4, 2, 1>"), (128, "wgrad_f32<2, 2, 2, 2>"), (192, "wgrad_f32<1, 4, 2, 1>")):
        rc, label = det_variant(desc(2, 24, 20, n, 64, 9, 1), "f32")
        assert rc == 0 and label.rsplit("+det", 1)[0] == inst, label


def _bad(base_kw, **kw):
    d = desc(**base_kw)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refusals(form):
    base = dict(B=2, H=24, W_=20, n=64, cin=64, ntaps=16 if form == "s16" else 9, a_step=1)
    d0 = desc(**base)
    al = 16 if form == "s16" else 8                        # bytes off the entry's operand alignment (32 / 16)
    st = 4 if form == "s16" else 2                         # floats off its stride granule (8 / 4)
    yield "n % 32", _bad(base, n=48)
    yield "n 0", _bad(base, n=0)
    yield "cin 48", _bad(base, cin=48)
    yield "cin 2", _bad(base, cin=2)
    yield "ntaps 7", _bad(base, ntaps=7)
    yield "ntaps 1 / cin 8", _bad(base, ntaps=1, cin=8)
    yield "a_step 3", _bad(base, a_step=3)
    yield "batch 0", _bad(base, batch=0)
    yield "height -1", _bad(base, height=-1)
    yield "M >= 2^31", _bad(base, batch=1 << 11, height=1 << 10, width=1 << 10)
    for p in ("g", "a", "dw", "zeros"):
        yield "null " + p, _bad(base, **{p: None})
    yield "g off alignment", _bad(base, g=d0.g + al)
    yield "a off alignment", _bad(base, a=d0.a + al)
    yield "zeros off alignment", _bad(base, zeros=d0.zeros + 4)
    for f in ("g_bs", "g_rs", "g_ps", "a_bs", "a_rs", "a_ps"):
        yield f + " off its granule", _bad(base, **{f: getattr(d0, f) + st})


@pytest.mark.parametrize("form", ["s16", "f32"])
def test_status_codes_are_those_of_the_atomics_entry(form):
    lib = _lib.load()
    seen = set()
    for what, d in _refusals(form):
        if form == "s16":
            want = W.variant(d)[0]                         # the atomics entry's checks, nothing launched
            atomic = lambda: lib.ammc_conv_wgrad_s16(C.byref(d), None, None)
            det = lambda: lib.ammc_conv_wgrad_s16_det(C.byref(d), None, 0x50000000, 1 << 40, None)
        else:
            atomic = lambda: lib.ammc_conv_wgrad_f32(C.byref(d), None)
            det = lambda: lib.ammc_conv_wgrad_f32_det(C.byref(d), 0x50000000, 1 << 40, None)
            want = None
        got_q = det_variant(d, form)[0]
        if want is None:
            if got_q == 0:                                  # (ntaps 1 / a_step 3 ...: what the fp32 entry takes, it takes too)
                continue
            want = atomic()                                 # refused before anything is launched
        assert got_q == want, (what, got_q, want)
        if want != 0:
            assert atomic() == want and det() == want, what
            assert det_floats(d, form) == 0 or "null" in what or "alignment" in what or "granule" in what, what
            seen.add(want)
    assert seen == {-1, -2}                                 # AMMC_EINVAL and AMMC_EUNSUP were both exercised
    for fn in (f"ammc_conv_wgrad_{form}_det_variant",):
        assert _q(fn, None)[0] == -1                        # null descriptor
        assert _q(fn, desc(2, 24, 20, 64, 64, 16, 1), n=16)[0] == -1          # short label buffer
        assert getattr(lib, fn)(C.byref(desc(2, 24, 20, 64, 64, 16, 1)), None, 96) == -1
    assert getattr(lib, f"ammc_conv_wgrad_{form}_det_floats")(None) == 0


@pytest.mark.parametrize("form", ["s16", "f32"])
def test_a_missing_or_short_workspace_is_refused_before_anything_is_launched(form):
    lib = _lib.load()
    d = desc(2, 24, 20, 64, 64, 16, 1)
    need = det_floats(d, form)
    assert need > 0
    if form == "s16":
        call = lambda ws, n: lib.ammc_conv_wgrad_s16_det(C.byref(d), None, ws, n, None)
    else:
        call = lambda ws, n: lib.ammc_conv_wgrad_f32_det(C.byref(d), ws, n, None)
    assert call(None, need) == -1 and call(0x50000000, need - 1) == -1 and call(0x50000000, 0) == -1


_CHILD = """
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_wgrad_det_host as T
out = {{}}
for form, grid in (("s16", T.s16_grid), ("f32", T.f32_grid)):
    for name, d in grid():
        out[name] = [T.det_variant(d, form), T.det_floats(d, form)]
print("LABELS " + json.dumps(out))
"""


@pytest.mark.parametrize("switch", ["AMMC_WGRAD_G11=1"])
def test_the_label_does_not_move_with_the_weight_gradient_switches(switch):
    """the switch is read once per process: a child with the switch set answers what this process answers"""
    env = {k: v for k, v in os.environ.items() if k not in W.SWITCHES}
    k, v = switch.split("=")
    env[k] = v
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout[r.stdout.index("LABELS ") + 7:].splitlines()[0])
    here = {}
    for form, grid in (("s16", s16_grid), ("f32", f32_grid)):
        for name, d in grid():
            here[name] = [list(det_variant(d, form)), det_floats(d, form)]
    assert got == here and len(here) > 250


# ammc_conv_wgrad_s16_slab_floats over the default grid of tests/wgrad_cases.py, as the library answered before the
# deterministic forms were added (floats; 0 = no slab form)
SLAB_FLOATS_BEFORE = {
    "r64-one-patch": 73728, "r64-run-crosses-columns-and-images": 73728, "r64-split-starts-mid-column": 147456,
    "r64-one-patch-columns": 147456, "r64-n192": 221184, "r128-one-patch": 73728, "r128-n256-cin128": 294912,
    "r128-crop": 221184, "o32-cout3": 73728, "o32-cout3-b2-8x64": 73728, "o32-cout3-slice": 73728,
    "first-cin8of3-n64": 24576, "first-cin16of12-n128-b3": 163840, "first-cin32-n64-b3": 147456,
    "first-cin8of3-n128-b3": 98304, "im2col-m63": 0, "im2col-n96": 0, "im2col-n32-h6": 0, "im2col-n160-cin16": 0,
    "im2col-cin8-kpad96": 0, "im2col-msplit3-short-last": 0, "c4-s2-cin8of3-n64": 0, "c4-s1-cin64-n32of1": 0,
    "c4-s2-odd-cin64-n64": 0, "c4-s1-cin8of3-n32of1": 0, "convt-exact-n128-co64": 0, "convt-odd-crop": 0,
    "convt-unscaled": 0, "place-r64-one": 147456, "place-r64-tiny": 147456, "place-r128-one": 147456,
    "place-r128-tiny": 147456, "place-o32-one": 73728, "place-o32-tiny": 73728, "place-first-one": 73728,
    "place-first-tiny": 73728, "place-im2col-one": 0, "place-im2col-tiny": 0,
}


def test_the_older_entries_did_not_move():
    if any(k in os.environ for k in W.SWITCHES):
        pytest.skip("the default table is checked in a process without the switches")
    lib = _lib.load()
    assert sorted(SLAB_FLOATS_BEFORE) == sorted(c.name for c in W.DEFAULT)
    for c in W.DEFAULT:
        d = W.desc(c)
        assert int(lib.ammc_conv_wgrad_s16_slab_floats(C.byref(d))) == SLAB_FLOATS_BEFORE[c.name], c.name
        assert W.variant(d) == (0, c.label), c.name                       # and the atomics entry's dispatch with them
        # every case the atomics entry takes, the deterministic entry takes: with the splits the descriptor says
        rc, label = det_variant(d, "s16")
        assert rc == 0 and label_k(label) == expected_splits(d, "s16"), (c.name, label)


def test_the_c_header_declares_the_six_entries():
    text = open(os.path.join(ROOT, "include", "ammc_hip.h")).read()
    for form in ("s16", "f32"):
        for tail in ("_det_floats", "_det", "_det_variant"):
            assert f"ammc_conv_wgrad_{form}{tail}(" in text
            assert hasattr(_lib.load(), f"ammc_conv_wgrad_{form}{tail}")


# ---- the switch above the library --------------------------------------------------------------------------------------------
def _base_args(tmp_path):
    return ["--rgb_root", str(tmp_path / "rgb"), "--op_root", str(tmp_path / "op"), "--out", str(tmp_path / "out"), "--iterations", "4"]


def test_run_train_parses_deterministic_and_refuses_a_resume_across_the_flag(tmp_path):
    from ammcnet_aaai2021_amd import run_train, train
    a = run_train.parse(_base_args(tmp_path))
    assert a.deterministic is False and run_train.deterministic_on(a) == train.DETERMINISTIC
    b = run_train.parse(_base_args(tmp_path) + ["--deterministic"])
    assert b.deterministic is True and run_train.deterministic_on(b) is True
    run_train.check_resume_deterministic({"deterministic": True}, b)
    if not train.DETERMINISTIC:
        run_train.check_resume_deterministic({"deterministic": False}, a)
        run_train.check_resume_deterministic({}, a)                         # a state from before the flag: not deterministic
        with pytest.raises(SystemExit, match="without --deterministic"):
            run_train.check_resume_deterministic({}, b)
        with pytest.raises(SystemExit, match="with --deterministic"):
            run_train.check_resume_deterministic({"deterministic": True}, a)


def test_the_models_carry_the_switch_and_it_defaults_to_the_environment():
    from ammcnet_aaai2021_amd import train, unet
    from ammcnet_aaai2021_amd.discriminator import PixelDiscriminator
    for m in (unet.UNet(12), unet.UNetMem_v7(12, 3), unet.twostream(12, 3, 6, 2), PixelDiscriminator(3, [128, 256, 512, 512])):
        assert m.deterministic is train.DETERMINISTIC
        assert "deterministic" not in m.state_dict()
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\nfrom ammcnet_aaai2021_amd import unet\n"
                        "print('DET', unet.UNetMem_v7(12, 3).deterministic)" % ROOT],
                       env=dict(os.environ, AMMC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "DET True" in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]


def test_the_engines_follow_the_switch_of_the_module_the_user_calls():
    """TrainEngine / DiscEngine / BlockEngine / MemoryBlockEngine are constructed without a device, whatever the switch says.
    `BlockEngine` / `MemoryBlockEngine` are built on a block (for `enc_quan_dec_res_topk`: on its inner `quan`); the
    switch they follow is the attribute of the module the user calls, AMMC_DETERMINISTIC only where that has none"""
    from ammcnet_aaai2021_amd import train, unet
    from ammcnet_aaai2021_amd.discriminator import DiscEngine, PixelDiscriminator
    G, D = unet.twostream(12, 3, 6, 2), PixelDiscriminator(3, [128, 256, 512, 512])
    for on in (False, True):
        G.deterministic = D.deterministic = on
        train.TrainEngine(G, "twostream")
        DiscEngine(D)
        assert train.deterministic_of(G) is on and train.deterministic_of(D) is on
    blk, res = unet.down(64, 128), unet.enc_quan_dec_res_topk(512, 64, 256, k=2)
    e_blk = train.BlockEngine(blk, "down", owner=blk)
    e_res = train.MemoryBlockEngine(res.quan, "vq_res", owner=res)
    assert e_blk.owner is blk and e_res.owner is res and e_res.module is res.quan
    assert train.MemoryBlockEngine(res.quan, "vq").owner is res.quan                 # no owner: the block itself
    assert train.deterministic_of(e_blk.owner) is train.DETERMINISTIC                  # no attribute: the environment's default
    blk.deterministic = res.deterministic = True
    assert train.deterministic_of(e_blk.owner) is True and train.deterministic_of(e_res.owner) is True
    train.BlockEngine(blk, "down", owner=blk)
    res.deterministic = False
    train.MemoryBlockEngine(res.quan, "vq_res", owner=res)
    assert train.deterministic_of(e_res.owner) is False and train.deterministic_of(e_blk.owner) is True
