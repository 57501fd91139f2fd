"""Host-side pieces of the data-parallel `run_train`: which resumes a train state allows, the row split of the one
global sampler stream, the new arguments, and the argument checks of the bucket entries (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from ammcnet_aaai2021_amd import _lib, pipeline as P, run_train


def _state(world, batch):
    return {"world": world, "args": {"batch": batch}}


def test_resume_keeps_the_global_batch_under_any_world():
    run_train.check_resume_batch(_state(2, 2), 1, 4)
    run_train.check_resume_batch(_state(2, 2), 4, 1)
    run_train.check_resume_batch(_state(2, 2), 2, 2)
    run_train.check_resume_batch({"args": {"batch": 4}}, 2, 2)          # a train state from before `world`: one rank
    with pytest.raises(SystemExit) as e:
        run_train.check_resume_batch(_state(2, 2), 2, 3)
    assert "global batch of 4" in str(e.value) and "this run has 6" in str(e.value)
    with pytest.raises(SystemExit):
        run_train.check_resume_batch(_state(2, 2), 1, 2)


@pytest.mark.parametrize("world, batch", [(1, 4), (2, 2), (4, 1), (3, 5)])
def test_rank_rows_of_one_global_draw(world, batch):
    """the union over ranks of rows [rank b, (rank + 1) b) of a `world x b` draw is the one-rank draw of `world x b`, in
    order, and leaves the stream where that draw leaves it - for both sampler classes"""
    def joint():
        return P.ClipSampler([12, 30, 9], [11, 29, 8], seed=2017)

    def single():
        return P.SingleClipSampler([12, 30, 9], 5, seed=2017, what="rgb")
    for make in (joint, single):
        ref = make()
        want = [ref.draw(world * batch) for _ in range(3)]
        after = ref.draw(1)
        ranks = [make() for _ in range(world)]
        for it in range(3):
            parts = [run_train.rank_rows(s.draw(world * batch), r, batch) for r, s in enumerate(ranks)]
            for col in range(len(want[it])):
                assert all(p[col].shape == (batch,) for p in parts)
                assert np.array_equal(np.concatenate([p[col] for p in parts]), want[it][col])
        for s in ranks:
            assert all(np.array_equal(x, y) for x, y in zip(s.draw(1), after))
    # world = 1: the split is the identity on today's draw
    one, again = joint(), joint()
    d = one.draw(4)
    assert all(np.array_equal(x, y) for x, y in zip(run_train.rank_rows(d, 0, 4), again.draw(4)))


def test_parse_takes_the_multi_rank_arguments():
    base = ["--rgb_root", "r", "--op_root", "o", "--out", "x", "--iterations", "1"]
    a = run_train.parse(base)
    assert a.dist_backend == "nccl" and a.sync_stats is False
    a = run_train.parse(base + ["--dist_backend", "gloo", "--sync_stats"])
    assert a.dist_backend == "gloo" and a.sync_stats is True
    with pytest.raises(SystemExit):
        run_train.parse(base + ["--dist_backend", "mpi"])


def test_a_multi_rank_start_must_name_its_ranks():
    assert run_train.launch_world({}) == 1 and run_train.launch_world({"WORLD_SIZE": "1"}) == 1
    assert run_train.launch_world({"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"}) == 2
    with pytest.raises(SystemExit, match="WORLD_SIZE=4 without RANK"):
        run_train.launch_world({"WORLD_SIZE": "4"})


def test_bucket_entries_reject_bad_tables_without_a_gpu():
    """argument errors of `ammc_bucket_pack_f32` / `ammc_bucket_unpack_scale_f32` are status codes decided on the host"""
    lib = _lib.load()
    assert C.sizeof(_lib.AmmcBucketTable) == 16 * _lib.AMMC_BUCKET_MAX == 2048
    t = _lib.AmmcBucketTable()
    t.ptr[:2] = [0x1000, 0x2000]
    t.end[:2] = [5, 12]
    ref = C.byref(t)
    assert lib.ammc_bucket_pack_f32(None, 2, 1, 0x100000, None) == -1
    assert lib.ammc_bucket_pack_f32(ref, 2, 1, None, None) == -1
    assert lib.ammc_bucket_pack_f32(ref, 0, 1, 0x100000, None) == -1
    assert lib.ammc_bucket_pack_f32(ref, _lib.AMMC_BUCKET_MAX + 1, 1, 0x100000, None) == -1
    assert lib.ammc_bucket_pack_f32(ref, 2, 2, 0x100000, None) == -1                # pad: 1 or 4
    assert lib.ammc_bucket_pack_f32(ref, 2, 4, 0x100004, None) == -1                # pad 4: flat on 16 bytes
    assert lib.ammc_bucket_unpack_scale_f32(ref, 2, 1, 0x100002, 0.5, None) == -1   # flat on 4 bytes
    t.end[1] = 5                                                                    # an empty member
    assert lib.ammc_bucket_unpack_scale_f32(ref, 2, 1, 0x100000, 0.5, None) == -1
    t.end[1] = 8                                                                    # ... also behind the padding
    assert lib.ammc_bucket_unpack_scale_f32(ref, 2, 4, 0x100000, 0.5, None) == -1
    t.end[1] = 12
    t.ptr[1] = 0x2002                                                               # a member off 4 bytes
    assert lib.ammc_bucket_pack_f32(ref, 2, 1, 0x100000, None) == -1
    t.ptr[1] = None
    assert lib.ammc_bucket_pack_f32(ref, 2, 1, 0x100000, None) == -1
