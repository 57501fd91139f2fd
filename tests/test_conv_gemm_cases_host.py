"""The case table of tests/conv_gemm_cases.py without a device: every case reaches the `ammc_conv_gemm_s16` instance it
claims (the library's own dispatch through `ammc_conv_gemm_s16_variant`, which launches nothing), the table covers every
instance the dispatcher has, and the CPU half of each GPU case - operands, fp64 truth, the fp32 witness, the sensitivity
of the truth to the lo halves - runs and meets the condition the S16 gate depends on."""
import os
import re

import pytest

import conv_gemm_cases as G
from conftest import ROOT


def dispatcher_families():
    """the tile instances `conv_gemm_s16_dispatch` can launch, parsed from its `launch<WGM, WGN, TM, TN>` calls
    (BM = 32 WGM TM, BN = 32 WGN TN), plus the split-K form of the instance its split-K branch launches"""
    text = open(os.path.join(ROOT, "ammcnet_aaai2021_amd", "csrc", "conv_gemm_s16.hip")).read()
    body = text[text.index("static int conv_gemm_s16_dispatch"):text.index('extern "C" int ammc_conv_gemm_s16(')]
    fams = set()
    for m in re.finditer(r"(a\.ksplit = ksp;\s*return )?launch<(\d+), (\d+), (\d+), (\d+)>", body):
        wgm, wgn, tm, tn = (int(v) for v in m.groups()[1:])
        fams.add("conv_gemm_s16<%dx%d>%s" % (32 * wgm * tm, 32 * wgn * tn, "+splitk" if m.group(1) else ""))
    return fams


def family(label: str) -> str:
    return re.sub(r"\+splitk\d+$", "+splitk", label)


def test_the_dispatcher_has_the_five_families_the_table_is_built_for():
    assert dispatcher_families() == {"conv_gemm_s16<128x128>", "conv_gemm_s16<128x128>+splitk", "conv_gemm_s16<256x128>",
                                     "conv_gemm_s16<128x64>", "conv_gemm_s16<128x32>"}


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_every_case_reaches_the_instance_it_claims(case):
    for ph in G.phases(case):
        if ph[3] > 0 and ph[4] > 0:
            assert G.s16_label(case, ph) == case.label, (case.name, ph)


def test_the_table_covers_every_instance_of_the_dispatcher():
    """an instance added to the dispatcher without a case fails here; so does a family whose cases were deleted"""
    reached = {family(c.label) for c in G.CASES}
    assert reached >= dispatcher_families(), dispatcher_families() - reached
    ks = {int(m.group(1)) for c in G.CASES for m in [re.search(r"\+splitk(\d+)$", c.label)] if m}
    assert len(ks) >= 2                                                     # at least two different split counts
    split = [c for c in G.CASES if "+splitk" in c.label]
    nchunks = lambda c: G.kpad(c) // 32
    assert any(nchunks(c) % int(c.label.rsplit("splitk", 1)[1]) for c in split)          # a slice count that does not divide K
    # one whose count is what the workspace allows, not what the shape asks for
    assert any(int(c.label.rsplit("splitk", 1)[1]) == c.splitk // (c.B * c.H * c.W * c.n) < min(nchunks(c) // 4, 512) for c in split)
    assert any(c.overflow for c in G.CASES)
    big = [c for c in G.CASES if c.label == G.L256]
    assert any((c.B * c.H * c.W) % 256 for c in big) and any((c.B * c.H * c.W) % 256 == 0 for c in big)
    assert all((c.B * c.H * c.W) % 128 for c in G.CASES if c.name.startswith("tail-"))


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_cpu_half_of_every_gpu_case(case):
    """operands, both fp64 truths and the witness evaluate on the CPU, and the S16 truth moves by at least ten gates when
    x loses its lo halves: a kernel that dropped a cross term could not pass the 2e-6 gate of this case"""
    h = G.host_half(case)
    ch, ho, wo, _, _ = G.out_geom(case)
    assert tuple(h["want_s16"].shape) == (case.B, ch, ho, wo)
    print(f"{case.name}: sensitivity to x.lo {h['sens']:.3e}, witness (torch fp32 vs fp64) {h['e_witness']:.3e}")
    assert h["sens"] >= G.SENS_MIN, h["sens"]
    assert 0.0 < h["e_witness"] < 1e-5
