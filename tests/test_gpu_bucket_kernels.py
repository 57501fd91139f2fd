"""`ammc_bucket_pack_f32` / `ammc_bucket_unpack_scale_f32` (csrc/bucket.hip) against `torch.cat` and `flat * scale` split
back, bit for bit, on member lists chosen where the kernels can go wrong - misaligned flat offsets, members of exactly one
chunk and one chunk + 1, one spanning many chunks, more members than one table holds - and the reducer on them against
its `torch._foreach_*` form in an RCCL world of one."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from ammcnet_aaai2021_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4096                       # floats per workgroup (BUCKET_CHUNK of csrc/bucket.hip)
MAXM = _lib.AMMC_BUCKET_MAX
GUARD = -777.25

CASES = {
    "odd_then_aligned": [1, 3, 5, 64],
    "chunk_and_chunk_plus_1": [CHUNK, CHUNK + 1, 8],
    "many_chunks": [300003],
    "two_launches": [1 + i % 7 for i in range(MAXM + 2)],
    "single_member": [17],
    "mixed": [1, 3, 5, 64, CHUNK, CHUNK + 1, 300003, 2, 4 * CHUNK],
}


def _members(sizes, seed=0):
    """every member a view into ONE guarded buffer: `gap` guard floats before each (1, 2, 3, 4, 1, ...: the members start
    at every alignment modulo 16 bytes) and after the last"""
    g = torch.Generator().manual_seed(seed)
    gaps = [1 + i % 4 for i in range(len(sizes) + 1)]
    buf = torch.full((sum(sizes) + sum(gaps),), GUARD)
    spans, off = [], 0
    for n, gap in zip(sizes, gaps):
        off += gap
        buf[off:off + n] = torch.randn(n, generator=g)
        spans.append((off, n))
        off += n
    buf = buf.to(DEV)
    return buf, [buf[o:o + n] for o, n in spans], spans


def _layout(sizes, pad):
    """the flat offset of every member's start (rounded up to `pad` floats) and the flat length - written out again
    here, so that the test does not inherit the reducer's arithmetic"""
    starts, off = [], 0
    for n in sizes:
        off = -(-off // pad) * pad
        starts.append(off)
        off += n
    return starts, off


def _run(entry, members, starts, pad, flat, *scale):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(0, len(members), MAXM):
        part = members[i:i + MAXM]
        t = _lib.AmmcBucketTable()
        t.ptr[:len(part)] = [m.data_ptr() for m in part]
        t.end[:len(part)] = [starts[i + j] + m.numel() - starts[i] for j, m in enumerate(part)]
        _lib.check(getattr(lib, entry)(C.byref(t), len(part), pad, flat.data_ptr() + 4 * starts[i], *scale, stream), entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("pad", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_pack_equals_cat_and_unpack_equals_scaled_split(case, pad):
    sizes = CASES[case]
    buf, members, spans = _members(sizes)
    before = buf.clone()
    starts, total = _layout(sizes, pad)
    # a flat buffer that starts off 16 bytes for pad = 1 (a later launch of a torch.cat-packed bucket does)
    store = torch.full((total + 8,), GUARD, device=DEV)
    lead = 3 if pad == 1 else 4
    flat = store[lead:lead + total]
    _run("ammc_bucket_pack_f32", members, starts, pad, flat)
    assert torch.equal(buf, before)                                           # the sources are only read
    if pad == 1:
        assert torch.equal(flat, torch.cat(members))
    want = torch.full_like(store, GUARD)                                      # padding and surroundings: never written
    for m, s in zip(members, starts):
        want[lead + s:lead + s + m.numel()] = m
    assert torch.equal(store, want)

    # the way back with scale = 1 / 3 into fresh guarded destinations
    src = torch.randn(total, generator=torch.Generator().manual_seed(1)).to(DEV)
    store[lead:lead + total] = src
    scale = 1.0 / 3.0
    buf.fill_(GUARD)
    _run("ammc_bucket_unpack_scale_f32", members, starts, pad, flat, scale)
    scaled = src * scale                                                      # one fp32 multiply, as `_foreach_mul_` does it
    want = torch.full_like(buf, GUARD)
    for (o, n), s in zip(spans, starts):
        want[o:o + n] = scaled[s:s + n]
    assert torch.equal(buf, want)                                             # members bit for bit, every guard untouched
    assert torch.equal(store[lead:lead + total], src)                         # the flat buffer is only read


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_reducer(port, q):
    try:
        os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist
        from ammcnet_aaai2021_amd import parallel as P
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        try:
            sizes = CASES["mixed"] + CASES["two_launches"] + [64, 128, 3]
            src = [torch.randn(n, generator=torch.Generator().manual_seed(i)).to(dev) for i, n in enumerate(sizes)]
            got = {}
            for hip in (True, False):
                # 30 KiB buckets: four per step, the last with more members (133) than a table holds
                red = P.BucketedGradReducer(bucket_mb=0.03, force=True, hip=hip)
                for step in range(2):                         # the second step reuses the flat buffers and layouts
                    grads = [t.clone() for t in src]
                    red.push(grads[:9])
                    red.push(grads[9:])
                    red.finish()
                    torch.cuda.synchronize()
                got[hip] = (grads, red.last_step_buckets)
            same = all(torch.equal(a, b) for a, b in zip(got[True][0], got[False][0]))
            ident = all(torch.equal(a, b) for a, b in zip(got[True][0], src))     # a world of one: the identity
            ok = same and ident and got[True][1] == got[False][1] >= 3
            q.put((ok, f"hip == foreach {same}, == input {ident}, buckets {got[True][1]} / {got[False][1]}"))
        finally:
            dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put((False, "".join(traceback.format_exception(type(e), e, e.__traceback__))[-1500:]))


def test_reducer_on_the_hip_kernels_equals_its_foreach_form_over_rccl():
    import queue
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_reducer, args=(_free_port(), q))
    p.start()
    res = None
    for _ in range(300):                               # a child that died without an answer fails the test at once
        try:
            res = q.get(timeout=1.0)
            break
        except queue.Empty:
            if not p.is_alive():
                break
    if p.is_alive():
        p.join(timeout=30)
    if p.is_alive():
        p.terminate()
    assert res is not None, f"the reducer worker exited with code {p.exitcode} before reporting"
    assert res[0], res
