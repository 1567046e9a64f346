"""The resumable MD5 chains on the GPU (flacgpu_md5_chains_*, csrc/kernels/md5_chain.inc): digests against hashlib.md5 of
the samples' low `width` bytes.  Every piece lies at an odd element offset of a device buffer whose other elements hold
0x7F filler: a kernel that read outside a piece and used what it found would hash the wrong bytes."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from test_md5_chain_host import check_samples, interesting_counts, le_bytes

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
FILL = 0x7F7F7F7F


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU visible to torch")
    return torch


def _L():
    from flac_codec_amd import _lib

    return _lib.lib()


class Chains:
    def __init__(self, n):
        self.n = n
        self.h = C.c_void_p()
        assert _L().flacgpu_md5_chains_create(-1, n, C.byref(self.h)) == 0

    def update(self, t, pieces, width, stream=None):
        """pieces: [(chain, off, count)] over the int32 device tensor t"""
        from flac_codec_amd import _lib

        tab = (_lib.Md5Piece * max(len(pieces), 1))()
        for p, (chain, off, count) in zip(tab, pieces):
            p.chain, p.off, p.count = chain, off, count
        return _L().flacgpu_md5_chains_update(self.h, t.data_ptr(), tab, len(pieces), width, stream)

    def final(self):
        out = (C.c_uint8 * (16 * max(self.n, 1)))()
        assert _L().flacgpu_md5_chains_final(self.h, out) == 0
        return [bytes(out[16 * i:16 * i + 16]) for i in range(self.n)]

    def close(self):
        _L().flacgpu_md5_chains_destroy(self.h)


def layout(arrays, first=1):
    """int32 arrays -> (host buffer with filler round every piece, [offset]): piece k starts at an element whose residue
    mod 4 walks through 1, 2, 3, 0, ..."""
    offs, at = [], first
    for k, a in enumerate(arrays):
        while at % 4 != (first + k) % 4:
            at += 1
        offs.append(at)
        at += len(a) + 3
    host = np.full(at + 8, FILL, dtype=np.uint32).view(np.int32)
    for off, a in zip(offs, arrays):
        host[off:off + len(a)] = a
    return host, offs


def md5(a, width):
    return hashlib.md5(le_bytes(a, width)).digest()


@pytest.mark.parametrize("n_chains", [1, 3, 65])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_one_call_against_hashlib(n_chains, width):
    torch = _torch()
    stage = _L().flacgpu_md5_stage_bytes()
    lens = [(7 * k * k + 13 * k + (0 if k % 9 else 5 * stage // width + 3)) % 9000 + (k == 0) * 4100 for k in range(n_chains)]
    arrays = [check_samples(n, first=1000 * k) for k, n in enumerate(lens)]
    host, offs = layout(arrays)
    t = torch.from_numpy(host).cuda()
    c = Chains(n_chains)
    assert c.update(t, [(k, offs[k], lens[k]) for k in range(n_chains)], width) == 0
    assert c.final() == [md5(a, width) for a in arrays]
    c.close()


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_lengths_round_the_padding_edges_and_the_staging_quantum(width):
    """one chain per length: every count up to 200 bytes and either side of one and two windows, all in one call; then
    the same pieces cut in two calls at a cut that leaves a partly filled buffer"""
    torch = _torch()
    counts = interesting_counts(width)
    arrays = [check_samples(n, first=17 * k) for k, n in enumerate(counts)]
    host, offs = layout(arrays, first=3)
    t = torch.from_numpy(host).cuda()
    want = [md5(a, width) for a in arrays]
    c = Chains(len(counts))
    assert c.update(t, [(k, offs[k], n) for k, n in enumerate(counts)], width) == 0
    assert c.final() == want
    cuts = [min(n, (5 * k + 1) % 97) for k, n in enumerate(counts)]
    assert c.update(t, [(k, offs[k], cuts[k]) for k in range(len(counts))], width) == 0
    assert c.update(t, [(k, offs[k] + cuts[k], n - cuts[k]) for k, n in enumerate(counts)], width) == 0
    assert c.final() == want
    c.close()


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_three_calls_a_short_middle_an_absent_chain_and_an_empty_piece(width):
    torch = _torch()
    a = [check_samples(3000, first=k) for k in range(4)]
    host, offs = layout(a)
    t = torch.from_numpy(host).cuda()
    c = Chains(4)
    first, mid = [1301, 40, 0, 2999], [63 // width, 1, 5, 0]   # middle pieces shorter than 64 bytes
    assert c.update(t, [(k, offs[k], first[k]) for k in (3, 1, 0, 2)], width) == 0          # (the table's order is free)
    assert c.update(t, [(k, offs[k] + first[k], mid[k]) for k in (0, 1, 3)], width) == 0    # chain 2 is absent; 3's is empty
    assert c.update(t, [(2, offs[2] + first[2], mid[2])], width) == 0
    rest = [(k, offs[k] + first[k] + mid[k], 3000 - first[k] - mid[k]) for k in range(4)]
    assert c.update(t, rest, width) == 0
    assert c.final() == [md5(x, width) for x in a]
    # a chain never fed gives the MD5 of the empty message; the chains are reusable after final
    assert c.update(t, [(1, offs[1], 3000)], width) == 0
    assert c.update(t, [], width) == 0
    got = c.final()
    assert got[1] == md5(a[1], width) and got[0] == got[2] == got[3] == hashlib.md5(b"").digest()
    c.close()


def test_refusals_change_no_state():
    torch = _torch()
    a = [check_samples(500, first=k) for k in range(2)]
    host, offs = layout(a)
    t = torch.from_numpy(host).cuda()
    c = Chains(2)
    assert c.update(t, [(0, offs[0], 100), (1, offs[1], 77)], 3) == 0
    assert c.update(t, [(0, offs[0] + 100, 400), (0, offs[0] + 100, 400)], 3) == INVALID_ARG   # a chain twice
    assert c.update(t, [(0, offs[0] + 100, 400), (1, offs[1] + 77, 423)], 5) == INVALID_ARG    # width 5
    assert c.update(t, [(0, offs[0] + 100, 400), (1, offs[1] + 77, 423)], 0) == INVALID_ARG
    assert c.update(t, [(2, offs[0], 1)], 3) == INVALID_ARG                                       # no such chain
    assert b"md5" in _L().flacgpu_last_error()
    assert c.update(t, [(0, offs[0] + 100, 400), (1, offs[1] + 77, 423)], 3) == 0
    assert c.final() == [md5(x, 3) for x in a]
    c.close()


def test_a_side_stream_and_one_long_chain():
    """the update is ordered on the caller's stream, final after it; 300 windows in one piece"""
    torch = _torch()
    n = 300 * _L().flacgpu_md5_stage_bytes() // 2 + 11
    a = check_samples(n)
    c = Chains(1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.full((n + 9,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        t[5:5 + n] = torch.from_numpy(a).cuda()
        assert c.update(t, [(0, 5, n // 3)], 2, stream=s.cuda_stream) == 0
        assert c.update(t, [(0, 5 + n // 3, n - n // 3)], 2, stream=s.cuda_stream) == 0
    assert c.final() == [md5(a, 2)]
    s.synchronize()
    c.close()
