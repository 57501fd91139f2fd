"""Per-layer references of the two auxiliary networks of the adversarial iteration, FlowNet2-SD
(ammcnet_aaai2021_amd/flownet.py) and PixelDiscriminator (ammcnet_aaai2021_amd/discriminator.py), and the readers that
bring an engine's retained buffers back "as the kernel sees them".  A helper module like tests/conv_gemm_cases.py, not a
test: tests/test_aux_refs_host.py checks it on the CPU, tests/test_gpu_flownet_layers.py and
tests/test_gpu_discriminator_layers.py check every layer of the engines against it.

Every reference is plain torch on CPU tensors, NCHW, in the dtype of its operands: float64 = the truth, float32 = the
witness of the fp32 gate (tests/test_gpu_conv_gemm.py).  Element-wise operations come from tests/stream_refs.py, the S16
encoding from tests/s16_codec.py.

The layer tables restate the two networks in logical tensor names; `flow_store` says where the engine keeps each of
them.  Nothing here imports the engines: the tables are compared with `_Engine._ensure_packs` and `DiscEngine.layers` by
the host test.  The checks themselves (`flow_check`, `flow_contracts`, `disc_check`, `disc_contracts`) live here too, on
CPU copies of the buffers, so that the host file can run them on buffers it fills itself - clean ones, and ones with the
faults planted that the device files are there to find."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_gemm_cases as G
import s16_codec as Q
import stream_refs as R
import wgrad_cases as WG

F64 = torch.float64
SLOPE = 0.1                                   # the networks' LeakyReLU slope as the reference states it
SLOPE32 = float(np.float32(0.1))              # ... and as the kernels hold it (a float argument)


# ---- per-layer operations ---------------------------------------------------------------------------------------------

def lrelu(y: torch.Tensor, slope: float = SLOPE) -> torch.Tensor:
    return torch.where(y > 0, y, y * slope)


def lrelu_bwd(y: torch.Tensor, g: torch.Tensor, slope: float = SLOPE) -> torch.Tensor:
    """g (y > 0 ? 1 : slope): the mask comes from the layer's own OUTPUT (both have the sign of the pre-activation)"""
    return torch.where(y > 0, g, g * slope)


def conv3(x, w, b=None, stride: int = 1, act: bool = False, slope: float = SLOPE):
    """Conv2d(k 3, stride 1 | 2, padding 1) + bias (+ LeakyReLU)"""
    y = F.conv2d(x, w, b, stride=stride, padding=1)
    return lrelu(y, slope) if act else y


def deconv4(x, w, b=None, act: bool = False, slope: float = SLOPE):
    """ConvTranspose2d(k 4, stride 2, padding 1) + bias (+ LeakyReLU); w [Cin, Cout, 4, 4]"""
    y = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    return lrelu(y, slope) if act else y


def conv4(x, w, b=None, stride: int = 2, act: bool = False, slope: float = SLOPE):
    """Conv2d(k 4, stride 1 | 2, padding 2) + bias (+ LeakyReLU)"""
    y = F.conv2d(x, w, b, stride=stride, padding=2)
    return lrelu(y, slope) if act else y


def _grads(fn, x, w, g):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = fn(x, w)
    assert y.shape == g.shape, (tuple(y.shape), tuple(g.shape))
    dx, dw = torch.autograd.grad(y, (x, w), g.to(y.dtype))
    return dx, dw, g.to(y.dtype).sum((0, 2, 3))


def conv3_grads(x, w, g, stride: int = 1):
    """(dx, dw, db) of conv3 for the gradient g of its (pre-activation) output, by autograd in the operands' dtype"""
    return _grads(lambda a, b: F.conv2d(a, b, None, stride=stride, padding=1), x, w, g)


def deconv4_grads(x, w, g):
    return _grads(lambda a, b: F.conv_transpose2d(a, b, None, stride=2, padding=1), x, w, g)


def conv4_grads(x, w, g, stride: int = 2):
    return _grads(lambda a, b: F.conv2d(a, b, None, stride=stride, padding=2), x, w, g)


# ---- the S16 view of a tensor --------------------------------------------------------------------------------------------

def s16_values(t: torch.Tensor) -> torch.Tensor:
    """what an fp32 tensor decodes to after the split (element-wise; a packed filter's image holds these values, which is
    how the convolution table gets `w` as the kernel sees it), float64"""
    hi, lo = Q.encode(t.detach().float().numpy())
    v = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / 2048.0
    return torch.from_numpy(v)


def hi_values(t: torch.Tensor) -> torch.Tensor:
    """the same with the lo halves dropped"""
    return t.detach().float().half().double()


def seen(t: torch.Tensor, s16: bool) -> torch.Tensor:
    """a parameter as a layer's kernel reads it, float64"""
    return s16_values(t) if s16 else t.detach().double()


# ---- readers of retained buffers ---------------------------------------------------------------------------------------------

class Stored:
    """a CPU copy of an engine `Act` (a channel slice of an NHWC buffer with a zero halo); `buf` is the WHOLE buffer"""

    def __init__(self, buf: torch.Tensor, B, H, W, c, c_off, halo):
        self.buf, self.B, self.H, self.W, self.c, self.c_off, self.halo = buf, B, H, W, c, c_off, halo

    def slice(self, c_off: int, c: int) -> "Stored":
        return Stored(self.buf, self.B, self.H, self.W, c, self.c_off + c_off, self.halo)

    def _interior(self) -> np.ndarray:
        h = self.halo
        return np.ascontiguousarray(self.buf.numpy()[:, h:h + self.H, h:h + self.W, self.c_off:self.c_off + self.c])

    def f32(self, c: Optional[int] = None) -> torch.Tensor:
        """NCHW float64 of an fp32 activation's first c channels"""
        v = torch.from_numpy(self._interior()).double().permute(0, 3, 1, 2)
        return (v if c is None else v[:, :c]).contiguous()

    def s16(self, c: Optional[int] = None) -> torch.Tensor:
        """NCHW float64 of an S16 activation (slice offset and width in whole groups of 8 channels)"""
        assert self.c_off % 8 == 0 and self.c % 8 == 0
        v = torch.from_numpy(Q.decode(self._interior())).permute(0, 3, 1, 2)
        return (v if c is None else v[:, :c]).contiguous()

    def values(self, s16: bool, c: Optional[int] = None) -> torch.Tensor:
        return self.s16(c) if s16 else self.f32(c)

    def put(self, v: torch.Tensor, s16: bool = False) -> None:
        """write NCHW values into the first channels of the slice's interior, as fp32 or as their S16 encoding (the host
        file's emulation of an engine; S16: whole groups of 8 channels, the rest of the last group zero)"""
        v = v.detach().float().permute(0, 2, 3, 1)
        c, h = v.shape[-1], self.halo
        if s16:
            cp = (c + 7) // 8 * 8
            assert self.c_off % 8 == 0 and cp <= self.c
            full = torch.zeros(*v.shape[:-1], cp)
            full[..., :c] = v
            v, c = torch.from_numpy(Q.words(full.numpy())).view(torch.float32), cp
        self.buf[:, h:h + self.H, h:h + self.W, self.c_off:self.c_off + c] = v

    def words(self) -> np.ndarray:
        """the whole buffer as int32 words"""
        return self.buf.numpy().view(np.int32)

    def halo_words(self) -> int:
        """number of non-zero 4-byte words in the halo of the WHOLE buffer (every channel)"""
        w, h = self.words(), self.halo
        inner = w[:, h:h + self.H, h:h + self.W]
        return int(np.count_nonzero(w)) - int(np.count_nonzero(inner))

    def channel_words(self, c0: int, c1: int, s16: bool = False) -> int:
        """number of non-zero words (S16: non-zero halves, hi or lo) in channels [c0, c1) of this slice, halo included"""
        if not s16:
            return int(np.count_nonzero(self.words()[..., self.c_off + c0:self.c_off + c1]))
        assert self.c_off % 8 == 0 and self.c % 8 == 0
        hi, lo = Q.unpack(np.ascontiguousarray(self.words()[..., self.c_off:self.c_off + self.c]))
        return int(np.count_nonzero(hi[..., c0:c1])) + int(np.count_nonzero(lo[..., c0:c1]))


def store(act, cache: Optional[dict] = None) -> Stored:
    """CPU copy of an engine Act; slices of one buffer share one copy through `cache`"""
    key = act.buf.data_ptr()
    if cache is not None and key in cache:
        buf = cache[key]
    else:
        buf = act.buf.detach().cpu().clone()
        if cache is not None:
            cache[key] = buf
    return Stored(buf, act.B, act.H, act.W, act.c, act.c_off, act.halo)


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max|got - want| / max|want|: the metric of every gate of the convolution and weight-gradient tables"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return float((got - want).abs().max() / want.abs().max())


# ---- FlowNet2-SD ---------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class FlowLayer:
    name: str                  # the engine's pack name (`_Engine._ensure_packs`)
    key: str                   # state_dict prefix of its weight / bias
    op: str                    # conv | deconv
    src: Tuple[str, ...]       # logical input tensors: more than one = the parts of a concatenation, in channel order
    dst: str                   # logical output tensor
    stride: int = 1
    act: bool = True
    f32_kernel: bool = False   # runs on the fp32 kernel in BOTH forms (the 2 -> 2 up-convolutions of the flow estimates)
    f32_out: bool = False      # S16 form: fp32 output from S16 operands (the flow heads)


def _flow_layers() -> List[FlowLayer]:
    out = [FlowLayer("conv0", "conv0.0", "conv", ("x0",), "c0")]
    prev = "c0"
    for lvl in range(1, 7):
        out.append(FlowLayer(f"conv{lvl}", f"conv{lvl}.0", "conv", (prev,), f"t{lvl}", stride=2))
        out.append(FlowLayer(f"conv{lvl}_1", f"conv{lvl}_1.0", "conv", (f"t{lvl}",), f"c{lvl}"))
        prev = f"c{lvl}"
    out.append(FlowLayer("predict_flow6", "predict_flow6", "conv", ("c6",), "f6", act=False, f32_out=True))
    cat = ("c6",)
    for lvl in (5, 4, 3, 2):
        out.append(FlowLayer(f"up{lvl + 1}", f"upsampled_flow{lvl + 1}_to_{lvl}", "deconv", (f"f{lvl + 1}",), f"u{lvl + 1}",
                             act=False, f32_kernel=True))
        out.append(FlowLayer(f"deconv{lvl}", f"deconv{lvl}.0", "deconv", cat, f"d{lvl}"))
        cat = (f"c{lvl}", f"d{lvl}", f"u{lvl + 1}")
        out.append(FlowLayer(f"inter_conv{lvl}", f"inter_conv{lvl}.0", "conv", cat, f"ic{lvl}", act=False))
        out.append(FlowLayer(f"predict_flow{lvl}", f"predict_flow{lvl}", "conv", (f"ic{lvl}",), f"f{lvl}", act=False,
                             f32_out=True))
    return out


FLOW_LAYERS = _flow_layers()
FLOW_BY_NAME = {L.name: L for L in FLOW_LAYERS}
FLOW_MULTI = [L for L in FLOW_LAYERS if len(L.src) > 1]
# logical channels of every tensor
FLOW_CH = dict(x0=6, c0=64, t1=64, c1=128, t2=128, c2=128, t3=256, c3=256, t4=512, c4=512, t5=512, c5=512, t6=1024, c6=1024,
               d5=512, d4=256, d3=128, d2=64, ic5=512, ic4=256, ic3=128, ic2=64,
               f6=2, f5=2, f4=2, f3=2, f2=2, u6=2, u5=2, u4=2, u3=2)
# (workspace key, channel offset, channels of the slice) of the tensors that live in a concatenation buffer; the flow part
# is a slice only in the fp32 form (S16: its own 8-channel buffers uf* -> u*)
_CAT = dict(c2=("cat2", 0, 128), d2=("cat2", 128, 64), c3=("cat3", 0, 256), d3=("cat3", 256, 128),
            c4=("cat4", 0, 512), d4=("cat4", 512, 256), c5=("cat5", 0, 512), d5=("cat5", 512, 512))
_CAT_U = dict(u3=("cat2", 192, 4), u4=("cat3", 384, 4), u5=("cat4", 768, 4), u6=("cat5", 1024, 4))


def flow_part_channels(L: FlowLayer) -> Tuple[int, ...]:
    return tuple(FLOW_CH[s] for s in L.src)


def flow_store(ws: dict, s16: bool) -> Dict[str, Stored]:
    """CPU copies of one workspace of `FlowNet2SD._engine.ws`, by logical name.  S16 form: `x0` / `u*` are the S16 tensors
    the layers read, `x0_f32` / `uf*` the fp32 tensors they were encoded from"""
    cache: dict = {}
    out: Dict[str, Stored] = {}
    for name in FLOW_CH:
        if name in _CAT:
            k, off, c = _CAT[name]
            out[name] = store(ws[k], cache).slice(off, c)
        elif name in _CAT_U and not s16:
            k, off, c = _CAT_U[name]
            out[name] = store(ws[k], cache).slice(off, c)
        elif name == "x0" and s16:
            out["x0"], out["x0_f32"] = store(ws["x0s"], cache), store(ws["x0"], cache)
        else:
            out[name] = store(ws[name], cache)
            if name in _CAT_U:
                out["uf" + name[1]] = store(ws["uf" + name[1]], cache)
    for k in ("cat2", "cat3", "cat4", "cat5"):
        out[k] = store(ws[k], cache)
    return out


def flow_is_s16_tensor(name: str, s16: bool) -> bool:
    """whether the logical tensor is kept as S16 in the given form: everything but the flow estimates f*"""
    return s16 and not name.startswith("f")


def flow_apply(L: FlowLayer, parts: Sequence[torch.Tensor], w: torch.Tensor, b: Optional[torch.Tensor], slope: float = SLOPE):
    """the layer on the concatenation of its parts, in the operands' dtype"""
    x = parts[0] if len(parts) == 1 else torch.cat(list(parts), 1)
    if L.op == "conv":
        return conv3(x, w, b, L.stride, L.act, slope)
    return deconv4(x, w, b, L.act, slope)


def flow_part_terms(L: FlowLayer, parts: Sequence[torch.Tensor], w: torch.Tensor, b: torch.Tensor) -> List[torch.Tensor]:
    """the pre-activation contribution of every part of a multi-part layer (the bias rides on part 0, as in the engine)"""
    out, c0 = [], 0
    for i, p in enumerate(parts):
        c = p.shape[1]
        if L.op == "conv":
            out.append(F.conv2d(p, w[:, c0:c0 + c], b if i == 0 else None, stride=L.stride, padding=1))
        else:
            out.append(F.conv_transpose2d(p, w[c0:c0 + c], b if i == 0 else None, stride=2, padding=1))
        c0 += c
    return out


def flow_frames(tag: str, shape) -> torch.Tensor:
    """frame pairs [B, 3, 2, H, W] in 0..255"""
    from ammcnet_aaai2021_amd import synthetic as S
    b, h, w = shape
    return (S.hashed_uniform(tag, (b, 3, 2, h, w)) + 1) * 127.5


def flow_chain(sd: dict, inputs: torch.Tensor, dtype=F64, slope: float = SLOPE, rgb_max=255.0, div_flow=20.0) -> Dict[str, torch.Tensor]:
    """the whole forward as a chain of the per-layer references: every logical tensor (NCHW) and `flow`"""
    t: Dict[str, torch.Tensor] = {}
    t["x0"] = R.flownet_prep(inputs, rgb_max).permute(0, 3, 1, 2).contiguous().to(dtype)
    for L in FLOW_LAYERS:
        w, b = sd[L.key + ".weight"].to(dtype), sd[L.key + ".bias"].to(dtype)
        t[L.dst] = flow_apply(L, [t[s] for s in L.src], w, b, slope)
    t["flow"] = R.upsample4(t["f2"].permute(0, 2, 3, 1), div_flow).to(dtype)
    return t


# ---- PixelDiscriminator ------------------------------------------------------------------------------------------------------

def disc_geometry(cin: int, filters: Sequence[int]) -> List[Tuple[int, int, int]]:
    """(cin, cout, stride) per layer: Conv2d(k 4, p 2, s 2) + LeakyReLU for filters[:-1], then the stride-1 head to 1 channel"""
    chans = [cin] + list(filters[:-1])
    return [(chans[i], chans[i + 1], 2) for i in range(len(chans) - 1)] + [(filters[-1], 1, 1)]


def disc_keys(n_layers: int) -> List[str]:
    return [f"net.{2 * i}" for i in range(n_layers)]


def disc_out_hw(h: int, stride: int) -> int:
    return (h + 4 - 4) // stride + 1


def disc_chain(sd: dict, x: torch.Tensor, wgt: torch.Tensor, dtype=F64, slope: float = SLOPE) -> dict:
    """forward and backward as a chain of the per-layer references.  acts[i] = input of layer i, out = the patch map,
    gs[i] = gradient of (out * wgt).sum() w.r.t. the PRE-activation output of layer i, dx, dw[i], db[i]"""
    keys = disc_keys(len([k for k in sd if k.endswith(".weight")]))
    n = len(keys)
    acts = [x.to(dtype)]
    for i, k in enumerate(keys[:-1]):
        acts.append(conv4(acts[i], sd[k + ".weight"].to(dtype), sd[k + ".bias"].to(dtype), 2, True, slope))
    out = conv4(acts[-1], sd[keys[-1] + ".weight"].to(dtype), sd[keys[-1] + ".bias"].to(dtype), 1, False)
    gs: List[Optional[torch.Tensor]] = [None] * n
    dw: List[Optional[torch.Tensor]] = [None] * n
    db: List[Optional[torch.Tensor]] = [None] * n
    gs[-1] = wgt.to(dtype)
    dx = None
    for i in reversed(range(n)):
        dx, dw[i], db[i] = conv4_grads(acts[i], sd[keys[i] + ".weight"].to(dtype), gs[i], 1 if i == n - 1 else 2)
        if i > 0:
            gs[i - 1] = lrelu_bwd(acts[i], dx, slope)
    return dict(acts=acts, out=out, gs=gs, dx=dx, dw=dw, db=db)


def grad_scale(g_buf: torch.Tensor) -> float:
    """the power of two by which the engine multiplies a gradient buffer before its S16 re-encoding
    (`ammc_absmax_bits_f32` + `ammc_split_rows_scaled_f32`: the maximum of the whole buffer lands in [1024, 2048))"""
    return Q.pow2_to_1024(Q.f32_bits(float(g_buf.abs().max())))


# ---- the cases of the two device files (the host file checks its conditions on the same inputs) -----------------------------------

FLOW_SHAPES = ((2, 64, 64), (3, 64, 128), (1, 128, 64))           # (B, H, W)
DISC_FILTERS = (128, 256, 512, 512)
DISC_CASES = (((2, 8, 8), DISC_FILTERS), ((3, 40, 72), DISC_FILTERS), ((1, 5, 7), DISC_FILTERS), ((2, 1, 9), DISC_FILTERS),
              ((2, 9, 11), (64, 128, 128)))


def flow_inputs(shape) -> torch.Tensor:
    return flow_frames("flow-layers-%dx%dx%d" % tuple(shape), shape)


def disc_inputs(shape, filters):
    """(x [B, 3, H, W], wgt on the patch map) of a discriminator case"""
    from ammcnet_aaai2021_amd import synthetic as S
    b, h, w = shape
    oh, ow = h, w
    for _, _, stride in disc_geometry(3, filters):
        oh, ow = disc_out_hw(oh, stride), disc_out_hw(ow, stride)
    tag = "disc-layers-%dx%dx%d-%d" % (b, h, w, len(filters))
    return S.hashed_uniform(tag + "x", (b, 3, h, w)), S.hashed_uniform(tag + "g", (b, 1, oh, ow))


# ---- the checks of the device files ------------------------------------------------------------------------------------------------
# A result is (name, error / gate, text); a check passes when error / gate <= 1.  Gates: GATE_S16 of the convolution table
# for everything an S16 kernel computes; the witness rule of tests/test_gpu_conv_gemm.py (e_hip <= 3 e_witness, the witness
# torch's fp32 CPU evaluation of the same layer on the same operands) for everything an fp32 kernel computes; GATE of the
# weight-gradient table for S16 weight gradients; the element-wise bounds of tests/test_gpu_stream_kernels.py for the prep,
# the x4 resize and the channel sum.

U32 = 2.0 ** -24


def gated(name: str, got: torch.Tensor, want: torch.Tensor, gate: float, witness: Optional[torch.Tensor] = None):
    if not bool(torch.isfinite(got).all()):
        return name, float("inf"), "an element is not finite"
    e = rel_err(got, want)
    if witness is None:
        return name, e / gate, f"err {e:.3e} gate {gate:.0e}"
    e_wit = rel_err(witness, want)
    return name, (e / (G.WITNESS_FACTOR * e_wit) if e_wit > 0 else (0.0 if e == 0 else float("inf"))), f"e_hip {e:.3e} e_witness {e_wit:.3e}"


def _bounded(name: str, got, want, bound):
    err = (got.double() - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return name, float(ratio.max()), "element-wise bound"


def flow_check_names() -> List[str]:
    return ["prep"] + [L.name for L in FLOW_LAYERS] + ["upsample"]


def flow_layer_check(L: FlowLayer, st: Dict[str, Stored], s16: bool, sd: dict):
    """one layer on its stored inputs against what it stored"""
    kernel_s16 = s16 and not L.f32_kernel
    parts = [st[s].values(flow_is_s16_tensor(s, s16), FLOW_CH[s]) for s in L.src]
    c = FLOW_CH[L.dst]
    if not s16 or L.f32_out:
        got = st[L.dst].f32(c)
    elif L.f32_kernel:
        got = st["uf" + L.dst[1]].f32(c)                     # the fp32 staging buffer of the up-sampled flow estimate
    else:
        got = st[L.dst].s16(c)
    w, b = seen(sd[L.key + ".weight"], kernel_s16), sd[L.key + ".bias"].double()
    want = flow_apply(L, parts, w, b, SLOPE32)
    wit = None if kernel_s16 else flow_apply(L, [p.float() for p in parts], w.float(), b.float(), SLOPE32)
    return gated(L.name, got, want, G.GATE_S16, wit)


def flow_check(st: Dict[str, Stored], s16: bool, x: torch.Tensor, out: torch.Tensor, sd: dict, rgb_max=255.0, div_flow=20.0):
    """every step of one forward: `x` the frame pairs given, `out` the flow returned, `st` the workspace afterwards"""
    b, _, _, h, w = x.shape
    res = []
    want = R.flownet_prep(x, rgb_max)
    xd = x.double()
    mean = xd.reshape(b, 3, -1).mean(-1).view(b, 3, 1, 1, 1)
    bound = 2 * (U32 * (mean.abs() + 2 * (xd - mean).abs()) / rgb_max).permute(0, 3, 4, 2, 1).reshape(b, h, w, 6)
    res.append(_bounded("prep", st["x0_f32" if s16 else "x0"].f32(6).permute(0, 2, 3, 1), want, bound))
    for L in FLOW_LAYERS:
        res.append(flow_layer_check(L, st, s16, sd))
    f2 = st["f2"].f32(2).permute(0, 2, 3, 1)
    assert tuple(out.shape) == (b, 2, h, w)
    res.append(_bounded("upsample", out, R.upsample4(f2, div_flow), 2 * 6 * U32 * R.upsample4(f2.abs(), div_flow)))
    assert [r[0] for r in res] == flow_check_names()
    return res


def flow_contracts(st: Dict[str, Stored], s16: bool) -> List[str]:
    """violations of the exact contracts of a workspace after a forward"""
    bad = [f"halo of {name} is not zero" for name, a in st.items() if a.halo_words() != 0]
    pads = [(f"f{v}", 2, 4, False) for v in (6, 5, 4, 3, 2)] + [("x0", 6, 8, s16)]
    if s16:
        pads += [(f"u{v}", 2, 8, True) for v in (6, 5, 4, 3)] + [(f"uf{v}", 2, 8, False) for v in (6, 5, 4, 3)] + [("x0_f32", 6, 8, False)]
    else:
        pads += [(f"u{v}", 2, 4, False) for v in (6, 5, 4, 3)]
    bad += [f"channels [{c0}, {c1}) of {name} are not zero" for name, c0, c1, enc in pads if st[name].channel_words(c0, c1, enc) != 0]
    if s16:
        for enc, src in [("x0", "x0_f32")] + [(f"u{v}", f"uf{v}") for v in (6, 5, 4, 3)]:
            if not np.array_equal(st[enc].words(), Q.words(st[src].buf.numpy())):
                bad.append(f"{enc} is not the S16 encoding of {src}")
    # the slices of a concatenation buffer are the logical tensors the layer checks read back: no channel goes unchecked
    for cat, names in (("cat5", ("c5", "d5", "u6")), ("cat4", ("c4", "d4", "u5")), ("cat3", ("c3", "d3", "u4")), ("cat2", ("c2", "d2", "u3"))):
        names = names[:2] if s16 else names
        offs = sorted((st[n].c_off, st[n].c) for n in names)
        whole = all(st[n].buf is st[cat].buf for n in names) and offs[0][0] == 0 and sum(o[1] for o in offs) == st[cat].c
        if not (whole and all(a[0] + a[1] == b[0] for a, b in zip(offs, offs[1:]))):
            bad.append(f"the slices of {cat} do not tile it")
    return bad


class DiscRun:
    """what a discriminator case leaves behind: sd, s16, layers [(cin, cout, stride, cin_p, gc)], acts / acts16 / gs / gs16
    (Stored), out, dx, grads {parameter name: gradient}, blocks [workgroups of the channel sum per layer], twins [(fp32, S16)
    pairs of packed filters]"""
    twins: list = []


def chan_sum_chain(m: int, c: int, blocks: int, u: int = 8) -> int:
    """additions on the longest chain of one partial row of ammc_chan_sum_f32 (`_chain` of tests/test_gpu_stream_kernels.py)"""
    py = 256 // (c // 4)
    trips = -(-m // (blocks * u * py))
    return trips * u + py - 1


def disc_check_names(n: int) -> List[str]:
    out = []
    for i in range(n):
        out += [f"fwd{i}", f"dW{i}", f"dgrad{i}+lrelu_bwd" if i > 0 else "dgrad0(x.grad)", f"db{i}"]
    return out


def disc_scales(r: DiscRun) -> List[float]:
    return [grad_scale(g.buf) if r.s16 else 1.0 for g in r.gs]


def disc_check(r: DiscRun):
    """every launch group of one forward and one backward"""
    s16, n = r.s16, len(r.layers)
    keys, scales, res = disc_keys(n), disc_scales(r), []
    for i, k in enumerate(keys):
        cin, cout, stride, _, gc = r.layers[i]
        last = i == n - 1
        w32, b32 = r.sd[k + ".weight"], r.sd[k + ".bias"]
        w, b = seen(w32, s16), b32.double()
        a_in = r.acts16[i].s16(cin) if s16 else r.acts[i].f32(cin)
        want = conv4(a_in, w, b, stride, not last, SLOPE32)
        got = r.out.double() if last else r.acts[i + 1].f32(cout)
        res.append(gated(f"fwd{i}", got, want, G.GATE_S16, None if s16 else conv4(a_in.float(), w32, b32, stride, not last, SLOPE32)))
        # backward from the gradient of the layer's pre-activation output as the kernels read it
        g_in = r.gs16[i].s16(cout) / scales[i] if s16 else r.gs[i].f32(cout)
        dx, dw, _ = conv4_grads(a_in, w, g_in, stride)
        wdx = wdw = None
        if not s16:
            wdx, wdw, _ = conv4_grads(a_in.float(), w32, g_in.float(), stride)
        res.append(gated(f"dW{i}", r.grads[k + ".weight"].double(), dw, WG.GATE, wdw))
        if i > 0:
            mask = r.acts[i].f32(cin)
            res.append(gated(f"dgrad{i}+lrelu_bwd", r.gs[i - 1].f32(cin), lrelu_bwd(mask, dx, SLOPE32), G.GATE_S16,
                             None if s16 else lrelu_bwd(mask.float(), wdx, SLOPE32)))
        else:
            res.append(gated("dgrad0(x.grad)", r.dx.double(), dx, G.GATE_S16, wdx))
        # bias gradient: the channel sum of the fp32 gradient buffer (both forms; the head's over 4 channels)
        g32 = r.gs[i].f32(cout)
        m = g32.shape[0] * g32.shape[2] * g32.shape[3]
        bound = 2 * (chan_sum_chain(m, gc if cout > 1 else 4, r.blocks[i]) + 1) * U32 * g32.abs().sum((0, 2, 3))
        res.append(_bounded(f"db{i}", r.grads[k + ".bias"], g32.sum((0, 2, 3)), bound))
    assert [x[0] for x in res] == disc_check_names(n)
    return res


def disc_contracts(r: DiscRun) -> List[str]:
    """violations of the exact contracts of the retained buffers after a backward"""
    s16 = r.s16
    groups = [("acts", r.acts), ("gs", r.gs)] + ([("acts16", r.acts16), ("gs16", r.gs16)] if s16 else [])
    bad = [f"halo of {name}[{i}] is not zero" for name, acts in groups for i, a in enumerate(acts) if a.halo_words() != 0]
    cin, _, _, cin_p, _ = r.layers[0]
    gc = r.layers[-1][4]
    if r.acts[0].channel_words(cin, cin_p) != 0 or (s16 and r.acts16[0].channel_words(cin, cin_p, True) != 0):
        bad.append("pad channels of the first input are not zero")
    if r.gs[-1].channel_words(1, gc) != 0 or (s16 and r.gs16[-1].channel_words(1, gc, True) != 0):
        bad.append("pad channels of the head's gradient are not zero")
    if s16:
        for i, scale in enumerate(disc_scales(r)):
            if not np.array_equal(r.acts16[i].words(), Q.words(r.acts[i].buf.numpy())):
                bad.append(f"acts16[{i}] is not the S16 encoding of acts[{i}]")
            if not np.array_equal(r.gs16[i].words(), Q.words((r.gs[i].buf * scale).numpy())):
                bad.append(f"gs16[{i}] is not the S16 encoding of gs[{i}] x {scale}")
        for j, (w32, w16) in enumerate(r.twins):
            if not np.array_equal(w16.numpy().view(np.int32), Q.words(w32.numpy().reshape(-1, 8)).reshape(w32.shape)):
                bad.append(f"packed filter twin {j} is not the S16 encoding of its fp32 filter")
    return bad
