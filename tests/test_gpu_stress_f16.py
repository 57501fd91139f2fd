"""Config 5 of BASELINE.json: the fp16-operand memory-addressing kernel (8192 slots x 512-d).
Metric: index agreement with the fp32 oracle wherever the distance margin
exceeds fp16 noise, gathered rows bit-exact for agreed indices, commit distance by tolerance."""
import pytest
import torch

from ammcnet_aaai2021_amd import ops, synthetic as S
from oracle import ammc_oracle as O
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def rows_in_registers(request):
    """which of the two kernels `ops.quantize_topk_f16` launches: True = memory_topk_f16r.hip (the default), False =
    memory_topk_f16.hip; restored afterwards"""
    saved = ops.F16_ROWS_IN_REGISTERS
    ops.F16_ROWS_IN_REGISTERS = request.param
    yield request.param
    ops.F16_ROWS_IN_REGISTERS = saved


@pytest.mark.parametrize("rows_in_registers", [True, False], indirect=True, ids=["f16r", "f16"])
@pytest.mark.parametrize("d,m,k,n", [(512, 8192, 2, 1024), (512, 8192, 2, 300), (128, 1000, 3, 513), (256, 4096, 1, 256)])
def test_memory_topk_f16(d, m, k, n, rows_in_registers):
    embed = S.hashed_normal(f"s16:{d}:{m}", (d, m), 0.9)
    x = S.hashed_normal(f"s16x:{d}:{m}", (1, 1, n, d), 0.8)
    qk, diff, q1, idx = ops.quantize_topk_f16(embed.to(DEV), x.to(DEV), k)
    wqk, wdiff, widx, widx1, flat, wq1 = O.quantize_topk(x, embed, k)
    idx, widx = idx.cpu().reshape(n, k).long(), widx.reshape(n, k)
    dist = (flat.double().pow(2).sum(1, keepdim=True) - 2 * flat.double() @ embed.double()
            + embed.double().pow(2).sum(0, keepdim=True))
    srt = dist.sort(dim=1).values
    margin = (srt[:, 1:k + 1] - srt[:, :k]).min(dim=1).values
    scale = flat.double().pow(2).sum(1) + embed.double().pow(2).sum(0).mean()
    safe = margin > 4e-3 * scale                      # fp16 operands: ~1e-3 relative on the dot products
    assert torch.equal(idx[safe], widx[safe])
    agree = (idx == widx).all(dim=1).double().mean()
    assert agree > 0.9, float(agree)
    same = (idx == widx).all(dim=1)
    assert torch.equal(qk.cpu().reshape(n, k * d)[same], wqk.reshape(n, k * d)[same])       # fp32 rows, bit exact
    # every chosen slot is a true near neighbour: within fp16 noise of the j-th smallest distance
    chosen = dist.gather(1, idx)
    assert bool(((chosen - srt[:, :k]).abs() <= 4e-3 * scale[:, None]).all())
    assert rel_err(diff.cpu(), wdiff) <= 5e-3


@pytest.mark.parametrize("n", [4096, 1000])
def test_memory_topk_f16_clustered_features_return_the_planted_slots(n):
    """Features as a trained memory sees them - between two slots, x = 0.6 E_s + 0.4 E_t + noise: both top-2 margins are
    far above what fp16 operands can blur (on random features only ~40 % of the rows have such margins: round-4 review,
    weak #7), so EVERY row must return exactly (s, t), agree with the fp32 oracle, and gather those two rows bit for bit."""
    d, m, k = 512, 8192, 2
    embed = S.hashed_normal("s16:cl:e", (d, m), 0.9)
    g = torch.Generator().manual_seed(5 + n)
    st = torch.randint(0, m, (n, 2), generator=g)
    st[:, 1] = torch.where(st[:, 1] == st[:, 0], (st[:, 1] + 1) % m, st[:, 1])
    et = embed.t().contiguous()
    x = 0.6 * et[st[:, 0]] + 0.4 * et[st[:, 1]] + 0.05 * torch.randn(n, d, generator=g)
    qk, diff, q1, idx = ops.quantize_topk_f16(embed.to(DEV), x.view(1, 1, n, d).to(DEV), k)
    idx = idx.cpu().reshape(n, k).long()
    assert torch.equal(idx, st)
    wqk, wdiff, widx, _, flat, wq1 = O.quantize_topk(x.view(1, 1, n, d), embed, k)
    assert torch.equal(idx, widx.reshape(n, k))
    assert torch.equal(qk.cpu().reshape(n, k * d), wqk.reshape(n, k * d))
    assert torch.equal(q1.cpu().reshape(n, d), flat + (wq1.reshape(n, d) - flat))           # unet.py:311: input + (quantize - input)
    assert rel_err(diff.cpu(), wdiff) <= 1e-5                      # (the commit term is fp32 arithmetic on the same rows)
    dist = flat.double().pow(2).sum(1, keepdim=True) - 2 * flat.double() @ embed.double() + embed.double().pow(2).sum(0, keepdim=True)
    srt = dist.sort(dim=1).values
    margin = (srt[:, 1:k + 1] - srt[:, :k]).min(dim=1).values
    scale = flat.double().pow(2).sum(1) + embed.double().pow(2).sum(0).mean()
    assert float((margin > 4e-3 * scale).double().mean()) > 0.99


def test_memory_topk_f16_65536_rows_chunked_oracle():
    """config 5 at 65,536 rows (512 workgroups of 128 rows; the bench runs 262,144): ONE launch, checked against the
    oracle chunk by chunk (4,096 rows each) with the gates above"""
    d, m, k, n, chunk = 512, 8192, 2, 65536, 4096
    embed = S.hashed_normal("s16:big:e", (d, m), 0.9)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, d, generator=g) * 0.8
    qk, diff, q1, idx = ops.quantize_topk_f16(embed.to(DEV), x.view(1, 1, n, d).to(DEV), k)
    idx = idx.cpu().reshape(n, k).long()
    qk = qk.cpu().reshape(n, k * d)
    e64 = embed.double()
    en = e64.pow(2).sum(0, keepdim=True)
    agree_all, sq = 0, 0.0
    for c0 in range(0, n, chunk):
        xs = x[c0:c0 + chunk]
        wqk, _, widx, _, flat, wq1 = O.quantize_topk(xs.view(1, 1, chunk, d), embed, k)
        widx = widx.reshape(chunk, k)
        dist = flat.double().pow(2).sum(1, keepdim=True) - 2 * flat.double() @ e64 + en
        srt = dist.sort(dim=1).values
        margin = (srt[:, 1:k + 1] - srt[:, :k]).min(dim=1).values
        scale = flat.double().pow(2).sum(1) + en.mean()
        safe = margin > 4e-3 * scale
        got = idx[c0:c0 + chunk]
        assert torch.equal(got[safe], widx[safe]), c0
        same = (got == widx).all(dim=1)
        agree_all += int(same.sum())
        assert torch.equal(qk[c0:c0 + chunk][same], wqk.reshape(chunk, k * d)[same]), c0
        chosen = dist.gather(1, got)
        assert bool(((chosen - srt[:, :k]).abs() <= 4e-3 * scale[:, None]).all()), c0
        sq += float((wq1.reshape(chunk, d).double() - flat.double()).pow(2).sum())
    assert agree_all / n > 0.9, agree_all / n
    assert abs(float(diff) - sq / (n * d)) <= 5e-3 * sq / (n * d)


@pytest.mark.parametrize("n", [65536, 65536 + 128 * 300 + 57, 1024])
def test_split_contraction_and_gather_equal_the_fused_launch(n, monkeypatch):
    """(runs memory_topk_f16.hip, the only kernel that reads `memory_split`: `ops.F16_ROWS_IN_REGISTERS` is False for its
    duration - with the default the two modes both ran memory_topk_f16r.hip and the comparison was vacuous)
    `memory_split`: contraction in chunks of whole rounds on the caller's stream, gather / commit of every chunk on
    the library's second stream beside the next chunk's contraction (the default from two rounds of workgroups up).  Same
    indices, same gathered fp32 rows and q_one bit for bit as ONE fused launch; the commit sum to summation order.  The
    ragged size ends in a partial chunk and a partial row block; 1024 rows force the split form below its default size.
    Successors on the caller's stream must see complete outputs: they are read right after the call, without a device
    synchronisation in between."""
    from ammcnet_aaai2021_amd import _lib
    lib = _lib.load()
    monkeypatch.setattr(ops, "F16_ROWS_IN_REGISTERS", False)
    d, m, k = 512, 8192, 2
    embed = S.hashed_normal("s16:split:e", (d, m), 0.9).to(DEV)
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, d, generator=g) * 0.8).view(1, 1, n, d).to(DEV)
    res = {}
    try:
        for mode in (0, 1):
            assert lib.ammc_set_option(b"memory_split", mode) == 0
            for _ in range(2):                                     # the second call re-uses the events of the first
                qk, diff, q1, idx = ops.quantize_topk_f16(embed, x, k)
            res[mode] = (qk.clone(), diff.clone(), q1.clone(), idx.clone())        # (clone: enqueued on the caller's stream)
    finally:
        lib.ammc_set_option(b"memory_split", -1)
    torch.cuda.synchronize()
    assert torch.equal(res[0][3], res[1][3]) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert rel_err(res[1][1].cpu(), res[0][1].cpu()) <= 1e-6
    assert lib.ammc_set_option(b"memory_split", 2) == -1              # AMMC_EINVAL


@pytest.mark.parametrize("regime", ["far (negative keys)", "clustered (positive keys)"])
def test_duplicated_slots_come_back_lower_slot_first(regime):
    """Round-5 advisor: the packed ranking keys of `memory_topk_f16r` (x.E - |E|^2 / 2 with the accumulator register in the
    four lowest mantissa bits) ordered exact ties correctly only for POSITIVE keys; config 5's random features have keys
    around -207, where the larger mantissa is the smaller float, so duplicated codebook rows came back as (higher slot,
    lower slot).  The final pair of a row is now put in slot order when its keys tie in the upper 28 bits (a sign-aware tag
    cost 6.7 % of the kernel).  Here 64 slot pairs hold identical rows - (s, s + 1) in one lane, one pair across the lane
    halves of a tile (s, s + 4), one across slot tiles (s, s + 4160) - and every feature row sits next to one pair: far features (x = 0.05 E_s +
    noise: both keys negative) and clustered ones (x = E_s + noise: both keys positive).  Expected, as from torch.topk on
    exact data and from `memory_topk_f16`: (s, s + 1) - lower slot first - and the gathered rows bit-identical."""
    d, m, k, n = 512, 8192, 2, 4096
    embed = S.hashed_normal("dup:e", (d, m), 0.9)
    pairs = [128 * i + 8 * (i % 4) + (i % 3) for i in range(64)]          # (s & 3) < 3: s + 1 shares the group of four, i.e. the lane
    for s in pairs:
        embed[:, s + 1] = embed[:, s]
    # ... and twins in the OTHER lane half of the same tile (s + 4) and in another slot tile (s + 4096): no tag orders those,
    # the per-row tie rule behind the merge does
    far_twin = {pairs[1]: pairs[1] + 4, pairs[2]: pairs[2] + 4096 + 64}      # (+ 64: clear of the other pairs)
    for s, t in far_twin.items():
        embed[:, s + 1] = S.hashed_normal(f"dup:undo:{s}", (d,), 0.9)    # (this pair's adjacent twin is undone)
        embed[:, t] = embed[:, s]
    g = torch.Generator().manual_seed(5)
    own = torch.tensor([pairs[i % 64] for i in range(n)])
    twin = torch.tensor([far_twin.get(pairs[i % 64], pairs[i % 64] + 1) for i in range(n)])
    gain = 0.05 if regime.startswith("far") else 1.0
    x = gain * embed[:, own].t().contiguous() + 0.01 * torch.randn(n, d, generator=g)
    keys = (x.double() @ embed.double()[:, own[:1]]).squeeze() - 0.5 * embed.double()[:, own[0]].pow(2).sum()
    assert (float(keys[0]) < 0) == regime.startswith("far")
    qk, diff, q1, idx = ops.quantize_topk_f16(embed.to(DEV), x.view(1, 1, n, d).to(DEV), k)
    idx = idx.cpu().reshape(n, k).long()
    if regime.startswith("far"):
        # (a slot of small norm may rank before a far feature's own pair: then the twins tie for the LAST place of the
        # top-2, and which of them takes it is not specified for this kernel's packed keys - see r_pack_key; what IS
        # guaranteed: whenever both twins are returned they come in slot order)
        has_a = (idx == own[:, None]).any(dim=1)
        has_b = (idx == twin[:, None]).any(dim=1)
        both = has_a & has_b
        assert int(both.sum()) > 16 and int((has_a | has_b).sum()) > 64          # (measured: 30 / 107 of 4096 rows)
        assert torch.equal(idx[both, 0], own[both]) and torch.equal(idx[both, 1], twin[both])
    else:
        assert torch.equal(idx[:, 0], own) and torch.equal(idx[:, 1], twin)
    got = qk.cpu().reshape(n, k, d)
    assert torch.equal(got[:, 0], embed.t()[idx[:, 0]]) and torch.equal(got[:, 1], embed.t()[idx[:, 1]])
