"""The case list of the many-stream MD5 sweep (tests/_md5_shapes.py) does what it is for.  CPU-only: the schedule model says which
populations the HASH tasks of csrc/host/coalesce.cpp would have hashed wrongly before they tested Md5::buffered(), and the batch
plan (flacenc_coalesce_plan, as tests/test_coalesce_plan.py) says that every such population meets ONE task the way the model
assumes -- one batch, every stream one segment, in the given order.  tests/test_gpu_md5_shapes.py then runs the cases."""
import pytest

import _md5_shapes as ms
from test_coalesce_plan import plan


def test_the_model_on_the_example_of_the_finding():
    # block 1000, mono, 16 bits: 2000 bytes a block = 16 mod 64; streams of 1, 5 and 5 blocks
    assert ms.sched([1, 5, 5], 2000) == [(3, 1, 16, 0, False), (2, 4, 0, 16, True)]
    assert ms.hazard([1, 5, 5], 2000)
    # whole MD5 blocks: lockstep from an aligned position at every step but the last chain's own
    assert ms.sched([1, 5, 6], 4096 * 2 * 3) == [(3, 1, 0, 0, True), (2, 4, 0, 0, True), (1, 1, 0, 0, False)]
    # 1001 x 2 x 16 (tests/test_gpu_segments.py): streams of 1 and 3 blocks never reach a lockstep step
    assert not ms.hazard([1, 3], 1001 * 2 * 2)
    # a stream without a whole block has no chain in the task
    assert ms.sched([0, 1, 5, 0, 5], 2000) == ms.sched([1, 5, 5], 2000)


@pytest.mark.parametrize("shape", ms.SHAPES, ids=ms.shape_id)
def test_the_tables_populations(shape):
    fb = ms.frame_bytes(shape)
    controls = [s for s in ms.SHAPES if ms.frame_bytes(s) % 64 == 0]
    assert len(controls) == 3
    if shape[3] is not None:
        assert fb % 64 != 0
        assert ms.hazard(shape[3], fb), "the table's population is not hazardous"
        for c in controls:
            assert not ms.hazard(shape[3], ms.frame_bytes(c))
        # ... and it is the smallest [a, b, b]
        a, b, _ = shape[3]
        smaller = [(x, y, y) for y in range(1, b + 1) for x in range(1, y) if (y, x) < (b, a)]
        assert not [p for p in smaller if ms.hazard(p, fb)]
    else:
        every = [(x, y, y) for y in range(1, ms.SOLO + 1) for x in range(1, y)]
        assert not [p for p in every if ms.hazard(p, fb)]
    if fb % 64 == 0:
        for _, blocks in ms.populations(ms.SHAPES.index(shape)):
            assert all(lock or live == 1 for live, _, _, _, lock in ms.sched(blocks[:ms.HASH_LANES], fb))


def test_frame_bytes_of_the_table():
    assert [ms.frame_bytes(s) % 64 for s in ms.SHAPES] == [16, 48, 48, 16, 40, 56, 40, 24, 36, 20, 52, 60, 58, 0, 0, 0]


@pytest.mark.parametrize("si,pi", ms.cases(), ids=[ms.case_id(si, pi) for si, pi in ms.cases()])
def test_every_population_is_one_batch_of_whole_streams(si, pi):
    """What run_hash meets: with the batch_frames the GPU test passes, the population is ONE batch, every stream with a whole block is
    one segment from its first block, in the given order -- so the 48-lane tasks are the model's."""
    shape = ms.SHAPES[si]
    _, blocks = ms.populations(si)[pi]
    segs, cap = plan(blocks, ms.batch_frames(blocks), shape[0] * shape[1])
    assert cap == sum(blocks)
    assert segs == [(k, 0, b, 0) for k, b in enumerate(blocks) if b]
    # the streams' lengths: one shorter than a block, about two of three with a short last block
    lens = ms.lengths(si, pi)
    assert [n // shape[0] for n in lens] == blocks
    assert lens[-1] < shape[0] and min(lens) >= 1
    tails = sum(1 for n in lens if n % shape[0])
    assert 0.6 * len(lens) <= tails <= 0.8 * len(lens), (tails, len(lens))


def test_enough_hazardous_pairs():
    haz = ms.hazardous_cases()
    assert len(haz) >= 10, len(haz)
    # every row with a population in the table, and some of the mixed ones; none at the controls
    assert all(ms.frame_bytes(ms.SHAPES[si]) % 64 for si, _ in haz)
    for si, shape in enumerate(ms.SHAPES):
        if shape[3] is not None:
            assert (si, 0) in haz
    mixed = [(si, pi) for si, pi in haz if ms.populations(si)[pi][0].startswith("mixed")]
    assert mixed, "no mixed population is hazardous"
    # a population of more than 48 streams is cut into two tasks, the second one of more than one chain
    for si in range(len(ms.SHAPES)):
        name, blocks = ms.populations(si)[-1]
        assert name == "big" and len([b for b in blocks if b]) >= 50
