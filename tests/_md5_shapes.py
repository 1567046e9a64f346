"""Stream shapes and populations for the many-stream MD5 sweep (tests/test_md5_shape_cases.py, tests/test_gpu_md5_shapes.py,
tools/soak/soak_many.py): block sizes, channel counts and sample widths whose frames are NOT whole 64-byte MD5 blocks, and sets of
stream lengths that make the coalescing front end's HASH tasks (csrc/host/coalesce.cpp run_hash) advance several chains in
lockstep from a position inside a block.

sched() restates the loop run_hash had before it asked Md5::buffered(): it took the lockstep branch (get_state ->
md5_blocks_groups -> set_state / add_blocks) whenever two or more chains were live and the step was a multiple of 64 bytes, also
when an earlier scalar step had left a partial block buffered -- those bytes were then hashed out of place.  The model stays as the
definition of a "hazardous" population: one that the old loop would have hashed wrongly."""
import numpy as np

HASH_LANES = 48      # chains per HASH task
SOLO = 32            # a stream of up to this many whole blocks is ONE segment, hashed by a HASH task
RATE = 44100

# (block, channels, bits, smallest hazardous population [a, b, b] in whole blocks per stream, or None)
SHAPES = [
    (1000, 1, 16, (1, 5, 5)),      # frame bytes = 16 mod 64
    (1000, 2, 24, (1, 5, 5)),      # 48
    (1000, 7, 16, (1, 5, 5)),      # 48
    (16, 1, 8, (1, 5, 5)),         # 16: the smallest legal block
    (1000, 1, 8, (1, 9, 9)),       # 40
    (1000, 1, 24, (1, 9, 9)),      # 56
    (500, 6, 20, (1, 9, 9)),       # 40
    (24, 1, 8, (1, 9, 9)),         # 24
    (1001, 2, 16, (1, 17, 17)),    # 36
    (1002, 2, 8, (1, 17, 17)),     # 20
    (333, 2, 16, (1, 17, 17)),     # 52
    (1150, 1, 16, (1, 17, 17)),    # 60
    (4095, 2, 24, None),           # 58: no hazard within 32 blocks; an odd shape that must simply be right
    (4096, 2, 24, None),           # 0: the controls -- the lockstep branch at every step
    (1152, 2, 24, None),
    (576, 1, 8, None),
]
MIXED = ((2, 10, 10, 32), (4, 4, 12, 20), (1, 2, 3, 4, 5, 6, 7, 8))
BIG_STREAMS = 52     # more than one 48-lane HASH task, more than one group of 16 SIMD lanes
BIG_BLOCKS = (1, 2, 5, 9, 17)   # gaps of 4, 8 and 16 blocks: lockstep steps at every frame size of the table


def shape_id(shape):
    return "%dx%dx%d" % shape[:3]


def frame_bytes(shape):
    block, channels, bits = shape[:3]
    return block * channels * ((bits + 7) // 8)


def sched(blocks, fb):
    """The steps of ONE HASH task over chains of `blocks` whole blocks of `fb` bytes, as the loop without the alignment test took
    them: [(live, common, bytes % 64, buffered_before, lockstep)].  Every live chain has taken the same bytes so far, so one
    `buffered` serves them all; a lockstep step leaves it as it was (add_blocks adds whole blocks), a scalar step adds its bytes."""
    left = [b for b in blocks if b > 0]
    steps, buffered = [], 0
    while left:
        common = min(left)
        nbytes = common * fb
        lockstep = len(left) >= 2 and nbytes % 64 == 0
        steps.append((len(left), common, nbytes % 64, buffered, lockstep))
        if not lockstep:
            buffered = (buffered + nbytes) % 64
        left = [b - common for b in left if b > common]
    return steps


def hazard(blocks, fb):
    """True if a lockstep step starts with a partial block buffered -- in any of the HASH tasks the solo streams of `blocks` are dealt
    to (48 at a time, in order; a stream without a whole block has no chain there)."""
    solo = [b for b in blocks if b > 0]
    assert all(b <= SOLO for b in solo)
    return any(lock and buffered
               for i in range(0, len(solo), HASH_LANES)
               for (_, _, _, buffered, lock) in sched(solo[i:i + HASH_LANES], fb))


def populations(si):
    """[(name, whole blocks per stream)] of shape SHAPES[si]: the table's smallest hazardous population, the three mixed ones, and
    one of BIG_STREAMS streams -- each followed by a stream shorter than a block (0 whole blocks)."""
    shape = SHAPES[si]
    out = []
    if shape[3] is not None:
        out.append(("min", list(shape[3]) + [0]))
    for k, m in enumerate(MIXED):
        out.append(("mixed%d" % k, list(m) + [0]))
    rng = np.random.Generator(np.random.PCG64(76000 + si))
    big = [int(v) for v in rng.choice(BIG_BLOCKS, BIG_STREAMS)]
    out.append(("big", big + [0]))
    return out


def batch_frames(blocks):
    """The batch_frames option that puts a whole population into one batch of the coalescing front end (it takes at least 64)."""
    return max(64, sum(blocks))


def lengths(si, pi):
    """Samples per channel of every stream of population pi of shape si: two streams of three end in a short last block of
    1 .. block - 1 samples (seeded), and so does the stream shorter than a block."""
    block = SHAPES[si][0]
    _, blocks = populations(si)[pi]
    rng = np.random.Generator(np.random.PCG64(77000 + 100 * si + pi))
    out = []
    for i, b in enumerate(blocks):
        tail = int(rng.integers(1, block)) if (i % 3 != 0 or b == 0) else 0
        out.append(b * block + tail)
    return out


def cases():
    """Every (shape index, population index) of the sweep."""
    return [(si, pi) for si in range(len(SHAPES)) for pi in range(len(populations(si)))]


def hazardous_cases():
    return [(si, pi) for si, pi in cases() if hazard(populations(si)[pi][1], frame_bytes(SHAPES[si]))]


def case_id(si, pi):
    return "%s-%s" % (shape_id(SHAPES[si]), populations(si)[pi][0])


# ---- total lengths that meet the MD5 padding's edges ---------------------------------------------------------------------------
RESIDUE_BLOCK = 192
RESIDUE_TARGETS = (0, 55, 56, 62, 63, 1, 2, 3, 4)
WIDTH_BITS = (16, 24, 32, 12, 20)      # 2, 3 and 4 bytes per sample; 12 and 20 bits hash as 2 and 3 bytes
ONE_SAMPLE_BITS = (8, 12, 16, 20, 24, 32)


def residue_lengths_8bit():
    """64 mono 8-bit streams: every residue of the total bytes mod 64, each a whole block and (but for the first) a short one."""
    return [RESIDUE_BLOCK + r for r in range(64)]


def residue_lengths(bits):
    """Mono sample counts (a whole block of RESIDUE_BLOCK and a short one) whose byte totals are the RESIDUE_TARGETS this width can
    reach, mod 64: [(target, samples)]."""
    w = (bits + 7) // 8
    out = []
    for t in RESIDUE_TARGETS:
        hit = [n for n in range(RESIDUE_BLOCK + 1, RESIDUE_BLOCK + 66) if (n * w) % 64 == t]
        if hit:
            out.append((t, hit[0]))
    return out
