"""The memory-addressing kernels, each alone through ctypes against the fp64 references of tests/memory_refs.py
(csrc/memory_topk.hip, memory_topk_s16.hip, memory_topk_f16.hip, memory_topk_f16r.hip, the codebook packers,
`ammc_pack_frag_rows_s16`, `ammc_sum_partials_f32`; shapes and inputs: tests/memory_cases.py).

"grid" / "planted" / "twins" inputs: every fp32 operation of the kernels is exact (tests/test_memory_refs_host.py proves
it), so indices, gathered rows, q_one and commit partials must EQUAL the reference - ties included, lower slot first; no row
is excluded.  "cont" inputs: B = `dist_error_bound`; every chosen slot's reference distance lies within B(chosen slot) + B(row's largest)
of the j-th smallest (all rows), the indices equal the reference wherever the first k + 1 sorted distances are more than
2 B(row's largest) apart (as a SET wherever only the gap behind the k-th is; `memory_refs.ambiguous_rows` says why the
row's largest), gathered rows and q_one are bit-equal to the fp32 expressions of the returned slots, partials lie within
gamma(chain) of the exact sum.  The worst error / bound ratios are printed (`RATIO ...`, run with -s).

Every output lives inside a larger buffer prefilled with a sentinel bit pattern, guard rows in front and behind: what the
kernel does not own must still hold it, and everything it owns must be written.  Inputs are finite (a row whose distances
are all NaN keeps the sentinel index 0x7fffffff and the gather would read out of bounds: a documented precondition)."""
import os

import pytest
import torch

from ammcnet_aaai2021_amd import _lib, synthetic as S
from ammcnet_aaai2021_amd.engine import Act, _ptr

import memory_cases as K
import memory_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
SENT = 0x7FA5A5A5                     # a NaN pattern no kernel produces; as an index, far beyond any slot
GUARD = 4                             # guard rows in front of and behind every output
EINVAL, EUNSUP = -1, -2
RESET = {"memory_rt": (0, (1, 2)), "memory_split": (-1, (0, 1))}        # the library's default, what the environment may force


def _reset_value(key):
    """what `key` held before a case set it: the library reads AMMC_<KEY> once (capi_misc.hip) and has no getter, so a
    session started with the variable set gets that value back, not the default"""
    default, allowed = RESET[key]
    env = os.environ.get("AMMC_" + key.upper(), "")
    return int(env) if env.lstrip("-").isdigit() and int(env) in allowed else default


def _s():
    return torch.cuda.current_stream().cuda_stream


def _sent(numel):
    t = torch.empty(numel, device=DEV, dtype=torch.int32)
    t.fill_(SENT)
    return t


def _ratio(kernel, what, worst):
    print(f"RATIO {kernel} {what} {worst:.4g}")


class Out:
    """idx [n][k], q_topk [n][k d], q_one [n][d], diff_partial [nb]: views inside sentinel buffers"""

    def __init__(self, n, dim, k, nb):
        self.n, self.dim, self.k, self.nb = n, dim, k, nb
        self.widths = {"idx": k, "q_topk": k * dim, "q_one": dim, "part": 1}
        self.rows = {"idx": n, "q_topk": n, "q_one": n, "part": nb}
        self.buf = {name: _sent((self.rows[name] + 2 * GUARD) * w) for name, w in self.widths.items()}

    def ptr(self, name):
        return self.buf[name].data_ptr() + 4 * GUARD * self.widths[name]

    def view(self, name):
        w = self.widths[name]
        return self.buf[name][GUARD * w:(GUARD + self.rows[name]) * w].view(self.rows[name], w)

    def check_extent(self, q_one=True):
        for name, w in self.widths.items():
            b, own = self.buf[name], self.view(name)
            assert bool((b[:GUARD * w] == SENT).all()) and bool((b[(GUARD + self.rows[name]) * w:] == SENT).all()), \
                f"{name}: written outside [0, {self.rows[name]}) rows"
            if name == "q_one" and not q_one:
                assert bool((own == SENT).all()), "q_one written although NULL was passed"
            else:
                assert not bool((own == SENT).any()), f"{name}: an element of the documented extent was left unwritten"

    def get(self):
        f = lambda name: self.view(name).cpu()
        return f("idx").long(), f("q_topk").view(torch.float32), f("q_one").view(torch.float32), f("part").view(torch.float32).view(-1)


class Codebook:
    """the operands of one codebook, packed by the library's own packers"""

    def __init__(self, lib, kernel, e):
        dim, m = e.shape
        self.e = e.to(DEV).contiguous()
        self.e_md = torch.empty(m, dim, device=DEV)
        self.enorm = torch.empty(m, device=DEV)
        _lib.check(lib.ammc_pack_codebook_f32(_ptr(self.e), dim, m, _ptr(self.e_md), _ptr(self.enorm), _s()), "pack_codebook")
        mp = R.mpad_of(m)
        if kernel == "s16":
            self.img = torch.empty(dim // 8 * 2 * mp * 8, device=DEV, dtype=torch.float16)
            _lib.check(lib.ammc_pack_codebook_s16(_ptr(self.e), dim, m, self.img.data_ptr(), _s()), "pack_codebook_s16")
        elif kernel == "f16":
            self.img = torch.empty(dim // 8 * mp * 8, device=DEV, dtype=torch.float16)
            self.enorm16 = torch.empty(m, device=DEV)
            _lib.check(lib.ammc_pack_codebook_f16(_ptr(self.e), dim, m, self.img.data_ptr(), _ptr(self.enorm16), _s()), "pack_f16")
        elif kernel == "f16r":
            self.img = torch.empty(lib.ammc_codebook_f16_tiles_bytes(dim, m), device=DEV, dtype=torch.uint8)
            _lib.check(lib.ammc_pack_codebook_f16_tiles(_ptr(self.e), dim, m, self.img.data_ptr(), _s()), "pack_f16_tiles")


def _blocks(lib, kernel, n):
    return {"f32": lib.ammc_memory_topk_blocks, "s16": lib.ammc_memory_topk_blocks, "f16": lib.ammc_memory_topk_f16_blocks,
            "f16r": lib.ammc_memory_topk_f16r_blocks}[kernel](n)


def _launch(lib, kernel, cb, x_d, k, out, q_one=True):
    n, dim = x_d.shape
    m = cb.e.shape[1]
    q1 = out.ptr("q_one") if q_one else None
    tail = (n, dim, m, k, out.ptr("idx"), out.ptr("q_topk"), q1, out.ptr("part"), _s())
    if kernel == "f32":
        rc = lib.ammc_memory_topk_fwd_f32(_ptr(x_d), _ptr(cb.e), _ptr(cb.e_md), _ptr(cb.enorm), *tail)
    elif kernel == "s16":
        rc = lib.ammc_memory_topk_fwd_s16(_ptr(x_d), cb.img.data_ptr(), _ptr(cb.e_md), _ptr(cb.enorm), *tail)
    elif kernel == "f16":
        rc = lib.ammc_memory_topk_fwd_f16(_ptr(x_d), cb.img.data_ptr(), _ptr(cb.e_md), _ptr(cb.enorm16), *tail)
    else:
        rc = lib.ammc_memory_topk_fwd_f16r(_ptr(x_d), cb.img.data_ptr(), _ptr(cb.e_md), *tail)
    _lib.check(rc, f"memory_topk {kernel}")


def _run(case):
    """both launches of a case (q_one given / NULL): (x, E, outputs of the first, diff) after the extent checks"""
    lib = _lib.load()
    n = K.rows(case, torch.cuda.get_device_properties(0).multi_processor_count)
    x, e = K.inputs(case, n)
    x_d = x.to(DEV)
    cb = Codebook(lib, case.kernel, e)
    nb = _blocks(lib, case.kernel, n)
    assert nb == -(-n // K.BLOCK[case.kernel])
    a, b = Out(n, case.d, case.k, nb), Out(n, case.d, case.k, nb)
    diff = _sent(8)
    try:
        for key, val in case.opt:
            assert lib.ammc_set_option(key.encode(), val) == 0
        _launch(lib, case.kernel, cb, x_d, case.k, a, True)
        _launch(lib, case.kernel, cb, x_d, case.k, b, False)
        _lib.check(lib.ammc_sum_partials_f32(a.ptr("part"), nb, 1.0 / float(n * case.d), diff.data_ptr() + 16, _s()), "sum_partials")
    finally:
        for key, _ in case.opt:
            lib.ammc_set_option(key.encode(), _reset_value(key))
    torch.cuda.synchronize()
    a.check_extent(True)
    b.check_extent(False)
    for name in ("idx", "q_topk", "part"):                 # q_one == NULL changes nothing else
        assert torch.equal(a.view(name), b.view(name)), f"{name} differs between the q_one and the q_one = NULL launch"
    assert bool((diff[:4] == SENT).all()) and bool((diff[5:] == SENT).all())
    return n, x, e, a.get(), float(diff[4:5].view(torch.float32).cpu())


def _reference(case, n, x, e):
    """`topk_ref` of the case's rows: (idx [n, k], the k + 1 smallest distances [n, <= k + 1], pick(slots [n, j]) -> their
    reference distances).  Grid and cont rows beyond `TILE_ROWS` repeat the first block (memory_cases.inputs), and so does
    the reference: it is computed once on the block, and no [n, m] matrix is built for the large cases"""
    nb = min(n, K.TILE_ROWS) if case.kind in ("grid", "cont") else n
    want, srt, dist = R.topk_ref(x[:nb], e, case.k, K.OPERAND[case.kernel])
    rm = torch.arange(n) % nb
    return want[rm], srt[:, :case.k + 1][rm], lambda slots: dist[rm[:, None], slots]


def _first(bad, *ts):
    rows_ = torch.nonzero(bad.reshape(bad.shape[0], -1).any(1)).flatten()[:4].tolist()
    return [(r, *[t[r].tolist() if t[r].numel() <= 8 else "..." for t in ts]) for r in rows_]


def _same_bits(got, want, what):
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first rows {torch.nonzero(bad.reshape(bad.shape[0], -1).any(1)).flatten()[:6].tolist()}"


def _ulps(a: float, b: float) -> int:
    t = torch.tensor([a, b], dtype=torch.float32).view(torch.int32).long()
    t = torch.where(t >= 0, t, -(t & 0x7FFFFFFF))
    return abs(int(t[0] - t[1]))


def _check_diff(case, n, part_gpu, diff_gpu):
    """`ammc_sum_partials_f32` = float(double sum of the partials x double(float(1 / (n d)))): the partials add exactly in
    double for as long as they have fewer than 2^29 of them; one rounding of the factor, one of the result"""
    v = float(part_gpu.double().sum()) / (n * case.d)
    assert abs(diff_gpu - v) <= (2 * U + (part_gpu.numel() + 2) * 2.0 ** -53) * abs(v)


@pytest.mark.parametrize("case", [c for c in K.TOPK_CASES if c.kind != "cont"], ids=lambda c: c.id)
def test_topk_exact_inputs_equal_the_reference(case):
    n, x, e, (idx, qk, q1, part), diff = _run(case)
    want, srt, pick = _reference(case, n, x, e)
    assert bool(((idx >= 0) & (idx < case.m)).all()), _first((idx < 0) | (idx >= case.m), idx)
    if K.packed_keys(case):
        # which of several exactly tied candidates takes the last place is open here; the distances are not, nor the order
        chosen = pick(idx)
        assert torch.equal(chosen, srt[:, :case.k]), _first(chosen != srt[:, :case.k], idx, want)
        tied = chosen[:, 1:] == chosen[:, :-1]
        assert bool((idx[:, 1:] > idx[:, :-1])[tied].all()), "tied slots out of slot order"
        assert bool((idx[:, 1:] != idx[:, :-1]).all())
        # ... and a row is open only if the k-th and the (k + 1)-th smallest distance tie: everywhere else the set is fixed
        # and ties inside it come in slot order, i.e. the reference's answer
        closed = srt[:, case.k] > srt[:, case.k - 1] if case.m > case.k else torch.ones(n, dtype=torch.bool)
        assert torch.equal(idx[closed], want[closed]), _first((idx != want) & closed[:, None], idx, want)
        if case.kind in ("planted", "twins"):             # the nearest slot (the lower twin of a pair) is never open
            assert torch.equal(idx[:, 0], want[:, 0])
    else:
        assert torch.equal(idx, want), _first(idx != want, idx, want)
    e_md = e.t().contiguous()
    _same_bits(qk, e_md[idx.reshape(-1)].reshape(n, -1), "q_topk")
    assert torch.equal(qk.double(), R.gather_ref(e, idx))
    w1, wpart, wdiff = R.commit_ref(x, e, idx, K.BLOCK[case.kernel])
    assert torch.equal(q1.double(), w1), _first(q1.double() != w1, idx)
    assert torch.equal(part.double(), wpart), (torch.nonzero(part.double() != wpart).flatten()[:6].tolist(), part[:4], wpart[:4])
    if K.is_pow2(n * case.d):
        assert diff == float(wdiff.float()), (diff, float(wdiff))
    else:
        assert _ulps(diff, float(wdiff)) <= 1, (diff, float(wdiff))
    if case.kind in ("planted", "twins"):
        assert bool((pick(idx[:, :1]) == 0).all())


@pytest.mark.parametrize("case", [c for c in K.TOPK_CASES if c.kind == "cont"], ids=lambda c: c.id)
def test_topk_cont_inputs_within_the_derived_bounds(case):
    n, x, e, (idx, qk, q1, part), diff = _run(case)
    op = K.OPERAND[case.kernel]
    want, srt, dist = R.topk_ref(x, e, case.k, op)
    k = case.k
    assert bool(((idx >= 0) & (idx < case.m)).all())
    bound = R.dist_error_bound(op, case.d, x, e, K.packed_keys(case))
    brow = bound.max(1).values
    chosen = dist.gather(1, idx)
    err = (chosen - srt[:, :k]).abs().max(1).values
    # the kernel's j-th smallest COMPUTED distance is within the row's largest bound of the reference's j-th smallest
    # (order statistics), and the chosen slot's reference distance within its own bound of its computed one
    bsel = bound.gather(1, idx).max(1).values + brow
    _ratio(case.kernel, f"distance {case.id}", float((err / bsel).max()))
    assert bool((err <= bsel).all()), _first((err > bsel)[:, None], idx, want)
    amb = R.ambiguous_rows(case.k, case.m, srt, bound)
    assert float(amb.double().mean()) <= 0.02
    assert torch.equal(idx[~amb], want[~amb]), _first((idx != want) & ~amb[:, None], idx, want)
    if case.m > k:                                           # the SET is fixed by the gap behind the k-th alone
        clear = (srt[:, k] - srt[:, k - 1]) > 2 * brow
        assert torch.equal(idx[clear].sort(1).values, want[clear].sort(1).values)
    assert bool((idx.sort(1).values[:, 1:] != idx.sort(1).values[:, :-1]).all()), "a slot returned twice"
    print(f"AMBIGUOUS {case.id} {float(amb.double().mean()):.4f} differing rows {int((idx != want).any(1).sum())}")
    # gathered rows, q_one: the fp32 data of the RETURNED slots, bit for bit
    e_md = e.t().contiguous()
    _same_bits(qk, e_md[idx.reshape(-1)].reshape(n, -1), "q_topk")
    e0 = e_md[idx[:, 0]]
    _same_bits(q1, x + (e0 - x), "q_one")
    # partials: terms (fl(E - x))^2 >= 0, each through `commit_chain` roundings, whatever the order
    split = dict(case.opt).get("memory_split") == 1
    chain = R.commit_chain("f16_split" if split else case.kernel, case.d, k)
    _, wpart, wdiff = R.commit_ref(x, e, idx, K.BLOCK[case.kernel])
    perr = (part.double() - wpart).abs()
    _ratio(case.kernel, f"partial {case.id}", float((perr / (R.gamma(chain) * wpart)).max()))
    assert bool((perr <= R.gamma(chain) * wpart).all())
    _check_diff(case, n, part, diff)


# ---- ammc_sum_partials_f32 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("count", K.SUM_COUNTS)
def test_sum_partials(count, kind):
    """out = float(S inv) with S the double sum of the partials (exact: < 2^29 fp32 terms of similar magnitude lose nothing
    in 53 bits on the grid; count 2^-53 relative otherwise) and inv = double(the fp32 argument): grid -> the same bits as
    that expression, cont -> u + count 2^-53"""
    lib = _lib.load()
    p = (R.grid(f"sump-{count}", (count,), 0, 4096, 64.0) if kind == "grid" else S.hashed_uniform(f"sump-{count}", (count,), 0.0, 300.0))
    inv = float(torch.tensor(1.0 / (count * 37), dtype=torch.float32))
    buf, out = _sent(count + 2 * GUARD), _sent(8)
    buf[GUARD:GUARD + count] = p.to(DEV).view(torch.int32)
    _lib.check(lib.ammc_sum_partials_f32(buf.data_ptr() + 4 * GUARD, count, inv, out.data_ptr() + 16, _s()), "sum_partials")
    torch.cuda.synchronize()
    assert bool((out[:4] == SENT).all()) and bool((out[5:] == SENT).all())
    got = float(out[4:5].view(torch.float32).cpu())
    v = float(p.double().sum()) * inv
    if kind == "grid":
        assert got == float(torch.tensor(v, dtype=torch.float64).float())
    else:
        assert abs(got - v) <= (U + 2 * count * 2.0 ** -53) * abs(v)


# ---- the packers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["grid", "cont"])
@pytest.mark.parametrize("dm", K.PACK_SHAPES, ids=lambda s: f"d{s[0]}-m{s[1]}")
def test_codebook_packers_equal_the_pack_references(dm, kind):
    """the four images bit for bit, padding slots included; the norms are sequential fp32 sums of d squares: exact on the grid,
    within gamma(d) of the exact norm otherwise"""
    lib = _lib.load()
    dim, m = dm
    e = R.grid(f"pk-{dim}-{m}", (dim, m)) if kind == "grid" else S.hashed_normal(f"pk-{dim}-{m}", (dim, m), 0.9)
    mp = R.mpad_of(m)
    e_d = e.to(DEV)
    e_md, enorm = _sent((m + 1) * dim), _sent(m + 1)
    s16, f16, en16 = _sent(dim // 8 * 2 * mp * 4 + 4), _sent(dim // 8 * mp * 4 + 4), _sent(m + 1)
    nbytes = lib.ammc_codebook_f16_tiles_bytes(dim, m)
    assert nbytes == (mp // 32) * (dim // 16 + 1) * 1024
    tiles = _sent(nbytes // 4 + 4)
    _lib.check(lib.ammc_pack_codebook_f32(_ptr(e_d), dim, m, e_md.data_ptr(), enorm.data_ptr(), _s()), "pack f32")
    _lib.check(lib.ammc_pack_codebook_s16(_ptr(e_d), dim, m, s16.data_ptr(), _s()), "pack s16")
    _lib.check(lib.ammc_pack_codebook_f16(_ptr(e_d), dim, m, f16.data_ptr(), en16.data_ptr(), _s()), "pack f16")
    _lib.check(lib.ammc_pack_codebook_f16_tiles(_ptr(e_d), dim, m, tiles.data_ptr(), _s()), "pack tiles")
    torch.cuda.synchronize()
    for t, own in ((e_md, m * dim), (enorm, m), (s16, dim // 8 * 2 * mp * 4), (f16, dim // 8 * mp * 4), (en16, m), (tiles, nbytes // 4)):
        assert bool((t[own:] == SENT).all()) and not bool((t[:own] == SENT).any())
    w_md, w_en = R.pack_f32_ref(e)
    w_f16, w_en16 = R.pack_f16_ref(e)
    w_frag, w_kb = R.pack_f16_tiles_ref(e)
    _same_bits(e_md[:m * dim].view(torch.float32).cpu().view(m, dim), w_md.float(), "embed_md")
    assert torch.equal(s16[:-4].cpu().view(torch.float16).view(dim // 8, 2, mp, 8).view(torch.int16), R.pack_s16_ref(e).view(torch.int16))
    assert torch.equal(f16[:-4].cpu().view(torch.float16).view(dim // 8, mp, 8).view(torch.int16), w_f16.view(torch.int16))
    img = tiles[:-4].cpu().view(mp // 32, (dim // 16 + 1) * 256)
    assert torch.equal(img[:, :dim // 16 * 256].contiguous().view(torch.float16).view(mp // 32, dim // 16, 64, 8).view(torch.int16),
                       w_frag.view(torch.int16))
    kb = img[:, dim // 16 * 256:].contiguous().view(torch.float32).double()
    real = torch.arange(mp).view(mp // 32, 32) < m
    assert torch.equal(kb[:, :32][~real], w_kb[:, :32][~real]) and not bool(kb[:, 32:].any())          # -3e38, zeros after float 32
    got = {"enorm": (enorm[:m].view(torch.float32).cpu().double(), w_en), "enorm16": (en16[:m].view(torch.float32).cpu().double(), w_en16),
           "tile constants": (-2.0 * kb[:, :32][real], w_en16)}
    for name, (g, w) in got.items():
        if kind == "grid":
            assert torch.equal(g, w), name
        else:
            worst = float(((g - w).abs() / (R.gamma(dim) * w)).max())
            _ratio("pack_codebook", f"{name} d{dim} m{m}", worst)
            assert worst <= 1.0, name


def test_guarded_pack_flags_what_the_hi_half_cannot_hold():
    lib = _lib.load()
    dim, m = 64, 40
    mp = R.mpad_of(m)
    for value, raised in ((65504.0, 0), (-65504.0, 0), (65520.0, 1), (float("inf"), 1), (float("-inf"), 1)):
        e = S.hashed_normal("pk-guard", (dim, m), 0.9)
        e[17, m - 1] = value
        img, flag = _sent(dim // 8 * 2 * mp * 4), torch.zeros(3, device=DEV, dtype=torch.int32)
        _lib.check(lib.ammc_pack_codebook_s16_guarded(_ptr(e.to(DEV)), dim, m, img.data_ptr(), flag.data_ptr() + 4, _s()), "guarded")
        torch.cuda.synchronize()
        assert flag.tolist() == [0, raised, 0], (value, flag.tolist())
        if not raised:
            assert torch.equal(img.cpu().view(torch.float16).view(dim // 8, 2, mp, 8).view(torch.int16), R.pack_s16_ref(e).view(torch.int16))


@pytest.mark.parametrize("nk", [(32, 8), (64, 128), (512, 128)])
def test_pack_frag_rows(nk):
    lib = _lib.load()
    n, k = nk
    w = S.hashed_uniform(f"frag-{n}-{k}", (n * k,), -4.0, 4.0)                  # any bit patterns: the kernel moves 16-byte pieces
    out = _sent(n * k + 4)
    _lib.check(lib.ammc_pack_frag_rows_s16(_ptr(w.to(DEV)), n, k, out.data_ptr(), _s()), "pack_frag_rows")
    torch.cuda.synchronize()
    assert bool((out[n * k:] == SENT).all())
    assert torch.equal(out[:n * k].cpu(), R.pack_frag_rows_ref(w, n, k))


# ---- ammc_memory_block_s16 -------------------------------------------------------------------------------------------------

def _s16_image(lib, t):
    """fp32 tensor -> its S16 image (same shape, as floats) by `ammc_split_rows_f32`"""
    src = t.to(DEV).contiguous()
    dst = torch.empty_like(src)
    _lib.check(lib.ammc_split_rows_f32(_ptr(src), src.numel(), _ptr(dst), _s()), "split_rows")
    return dst


def _s16_decode(img):
    """S16 image [..., c] floats -> (hi, lo) fp64 [..., c]"""
    hl = img.cpu().contiguous().view(torch.float16).view(*img.shape[:-1], img.shape[-1] // 8, 2, 8).double()
    return hl[..., 0, :].reshape(*img.shape), hl[..., 1, :].reshape(*img.shape)


def _packed_filter(lib, w, cout, cin):
    """[cout][cin] -> `ammc_pack_conv_weight_f32` (1x1) -> S16 rows"""
    out = torch.empty(cout, cin, device=DEV)
    _lib.check(lib.ammc_pack_conv_weight_f32(_ptr(w.to(DEV).contiguous()), cout, cin, 1, cin, _ptr(out), _s()), "pack_conv_weight")
    return _s16_image(lib, out)


@pytest.mark.parametrize("spec", K.BLOCK_CASES, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in K.BLOCK_CASES])
def test_memory_block(spec):
    """grid / planted: y, idx, q_topk, q_one, diff_partial and diff equal `block_ref`; *counter is zero after each of two
    launches, *overflow_flag untouched, nothing outside the documented extents written.
    cont: the reference starts from the S16 operands' VALUES (hi + lo / 2048 of x, enc_w, dec_w: what the kernel is given);
    the bounds on z, the distances, q_one, the partials and y are `memory_refs.block_*_bound`, derived there."""
    kind, (b, h, w), m = spec
    lib = _lib.load()
    c, dim, k = 512, 64, 2
    n = b * h * w
    x, enc_w, enc_b, e, dec_w, dec_b = K.block_inputs(kind, (b, h, w), m)
    X = Act(torch.zeros(b, h + 2, w + 2, c, device=DEV), b, h, w, c, 0, 1)
    X.interior().copy_(_s16_image(lib, x))
    ybuf = _sent(b * (h + 2) * (w + 2) * c).view(torch.float32).view(b, h + 2, w + 2, c)
    Y = Act(ybuf, b, h, w, c, 0, 1)
    enc16, dec16 = _packed_filter(lib, enc_w, dim, c), _packed_filter(lib, dec_w, c, k * dim)
    dec_wf = torch.empty_like(dec16)
    _lib.check(lib.ammc_pack_frag_rows_s16(_ptr(dec16), c, k * dim, _ptr(dec_wf), _s()), "pack_frag_rows")
    cb = Codebook(lib, "s16", e)
    eb, db = enc_b.to(DEV), dec_b.to(DEV)
    nb = lib.ammc_memory_topk_blocks(n)
    outs = [Out(n, dim, k, nb), Out(n, dim, k, nb)]
    diff, state = _sent(8), torch.zeros(8, device=DEV, dtype=torch.int32)             # state[2] = counter, state[5] = overflow flag
    counters = []
    for o in outs:
        _lib.check(lib.ammc_memory_block_s16(X.pix0(), *X.strides, Y.pix0(), *Y.strides, b, h, w, c, _ptr(enc16), _ptr(eb),
                                             cb.img.data_ptr(), _ptr(cb.e_md), _ptr(cb.enorm), dim, m, k, _ptr(dec_wf), _ptr(db),
                                             o.ptr("idx"), o.ptr("q_topk"), o.ptr("q_one"), o.ptr("part"), diff.data_ptr() + 16,
                                             state.data_ptr() + 8, state.data_ptr() + 20, _s()), "memory_block")
        torch.cuda.synchronize()
        counters.append(state.tolist())
    assert counters == [[0] * 8, [0] * 8], counters                        # counter back at zero, flag and neighbours untouched
    assert bool((diff[:4] == SENT).all()) and bool((diff[5:] == SENT).all())
    for o in outs:
        o.check_extent(True)
    for name in ("idx", "q_topk", "q_one", "part"):
        assert torch.equal(outs[0].view(name), outs[1].view(name)), name
    own = torch.zeros(ybuf.shape, dtype=torch.bool, device=DEV)
    own[:, 1:1 + h, 1:1 + w] = True
    ybits = ybuf.view(torch.int32)
    assert bool((ybits[~own] == SENT).all()) and not bool((ybits[own] == SENT).any())
    idx, qk, q1, part = outs[0].get()
    got_diff = float(diff[4:5].view(torch.float32).cpu())
    yhi, ylo = _s16_decode(Y.interior())
    e_md = e.t().contiguous()
    _same_bits(qk, e_md[idx.reshape(-1)].reshape(n, -1), "q_topk")
    case = K.Case("s16", kind, n, dim, m, k)
    if kind != "cont":
        r = R.block_ref(x, enc_w, enc_b, e, dec_w, dec_b, k)
        assert torch.equal(idx, r["idx"]), _first(idx != r["idx"], idx, r["idx"])
        assert torch.equal(q1.double(), r["q_one"]) and torch.equal(part.double(), r["diff_partial"])
        whi, wlo = R.s16_split(r["y"].float())
        assert torch.equal(yhi, whi) and torch.equal(ylo, wlo)
        assert torch.equal(yhi + ylo / R.S_LO, r["y"])
        if K.is_pow2(n * dim):
            assert got_diff == float(r["diff"].float())
        else:
            assert _ulps(got_diff, float(r["diff"])) <= 1
        return
    xv, ew, dw = (hl[0] + hl[1] / R.S_LO for hl in (_s16_decode(X.interior()), _s16_decode(enc16), _s16_decode(dec16)))
    r = R.block_ref(xv, ew, enc_b, e, dw, dec_b, k, round_z=False)
    z, xr = r["z"], xv.reshape(n, c)
    bz = R.block_z_bound(xr, ew, enc_b)
    bound = R.block_dist_bound(z, e, bz)
    brow = bound.max(1).values
    err = (r["dist"].gather(1, idx) - r["srt"][:, :k]).abs().max(1).values
    bsel = bound.gather(1, idx).max(1).values + brow
    _ratio("memory_block", f"distance {spec}", float((err / bsel).max()))
    assert bool((err <= bsel).all())
    # z's worst-case bound rides on every distance, so more rows are ambiguous than in the rankers' own cases; the share is
    # a property of the inputs, capped by tests/test_memory_refs_host.py: at least 75 % of the rows are compared
    amb = R.ambiguous_rows(k, m, r["srt"], bound)
    print(f"AMBIGUOUS memory_block {spec} {float(amb.double().mean()):.4f} differing rows {int((idx != r['idx']).any(1).sum())}")
    assert float(amb.double().mean()) <= K.BLOCK_AMBIGUOUS_CAP
    assert torch.equal(idx[~amb], r["idx"][~amb])
    e0 = e_md[idx[:, 0]].double()
    q1b = R.block_q_one_bound(z, e0, bz)
    q1err = (q1.double() - (z + (e0 - z))).abs()
    _ratio("memory_block", f"q_one {spec}", float((q1err / q1b).max()))
    assert bool((q1err <= q1b).all())
    wpart, pb = R.block_partial_bound(z, e0, bz, nb, R.commit_chain("block", dim, k))
    _ratio("memory_block", f"partial {spec}", float(((part.double() - wpart).abs() / pb).max()))
    assert bool(((part.double() - wpart).abs() <= pb).all())
    _check_diff(case, n, part, got_diff)
    qv = e_md[idx.reshape(-1)].reshape(n, k * dim).double()
    ywant = qv @ dw.t() + dec_b.double() + xr
    by = R.block_y_bound(qv, dw, dec_b, xr, ywant)
    yerr = ((yhi + ylo / R.S_LO).reshape(n, c) - ywant).abs()
    _ratio("memory_block", f"y {spec}", float((yerr / by).max()))
    assert bool((yerr <= by).all())


# ---- refusals: documented return codes of calls that launch nothing ---------------------------------------------------------

def test_refusals():
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()

    def f32(n, d, m, k):
        return lib.ammc_memory_topk_fwd_f32(p, p, p, p, n, d, m, k, p, p, p, p, _s())

    def s16(n, d, m, k):
        return lib.ammc_memory_topk_fwd_s16(p, p, p, p, n, d, m, k, p, p, p, p, _s())

    def f16(n, d, m, k):
        return lib.ammc_memory_topk_fwd_f16(p, p, p, p, n, d, m, k, p, p, p, p, _s())

    def f16r(n, d, m, k, tiles=p):
        return lib.ammc_memory_topk_fwd_f16r(p, tiles, p, n, d, m, k, p, p, p, p, _s())

    for fn, d_ok, d_bad in ((f32, 64, 96), (s16, 64, 96), (f16, 128, 96), (f16r, 128, 96)):
        assert fn(8, d_ok, 3, 4) == EINVAL                      # k > m
        assert fn(8, d_ok, 16, 5) == EUNSUP                     # k = 5
        assert fn(8, d_bad, 16, 2) == EUNSUP                    # d = 96
        assert fn(0, d_ok, 16, 2) == EINVAL
    assert f16r(8, 128, 16, 2, tiles=p + 8) == EINVAL           # a misaligned `tiles` pointer
    assert lib.ammc_pack_codebook_f16_tiles(p, 128, 16, p + 8, _s()) == EINVAL
    assert lib.ammc_pack_frag_rows_s16(p, 48, 128, p, _s()) == EINVAL

    def block(m, k=2, d=64, c=512):
        return lib.ammc_memory_block_s16(p, 512 * 64, 512 * 8, 512, p, 512 * 64, 512 * 8, 512, 1, 8, 8, c, p, p, p, p, p, d, m, k, p, p,
                                         p, p, p, p, p, p, p, _s())
    assert block(2049) == EUNSUP and block(64, k=3) == EUNSUP and block(64, c=256) == EUNSUP and block(1, k=2) == EINVAL
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing was launched
