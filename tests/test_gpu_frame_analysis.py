"""Frame analysis on the device: flacgpu_decoder_plan_analysis / flacgpu_decoder_analyze (k_analyze_many) behind every
scan, against the Python model of the rule (_frame_model), the choices _flacsyn wrote, and the oracle's own plans
(_analysis_cases, _compare.compare_frame).  test_frame_analysis_host.py holds the model to its references and the host
rule to the model without a device; here the device is held to the same.  Every batch is small: a few hundred frames
of at most 4608 samples, one or two kernel passes each."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _analysis_cases as ac
import _compare as cmp
import _flacsyn as fs
import _foreign_matrix as fmx
import _frame_model as model

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, TOO_SMALL = 0, -1, -5
GUARD, FILL = 256, 0xA5   # guard bytes in front of, between and behind the three outputs


@pytest.fixture(scope="module")
def dec():
    from flac_codec_amd.gpu import Decoder

    d = Decoder(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def model_of(frame_bytes, bps):
    return model.parse_frame(frame_bytes, bps)


def case_entries(cases):
    """One entry per frame, in batch order: (where, frame bytes, STREAMINFO sample size, oracle (plan, planar) or None)."""
    out = []
    for case in cases:
        for k, fb in enumerate(case.frame_bytes):
            ref = (case.plans[k], case.planar[k]) if hasattr(case, "plans") else None
            out.append((f"{case.name} frame {k}", fb, case.bps, ref))
    return out


def analyze_guarded(dec, rows=True, device=True):
    """flacgpu_decoder_analyze of the scanned batch into one buffer that holds guard bytes, the frames, guard bytes, the
    subframes, guard bytes, the rows, guard bytes -- in device or host memory.  Returns a FrameAnalysis with numpy
    arrays; asserts that every guard byte is intact."""
    import torch

    from flac_codec_amd import _lib, gpu

    nf, ns, nr = dec.plan_analysis()
    fb, sb, rb = nf * gpu.ANALYSIS_FRAME_DTYPE.itemsize, ns * gpu.SUBFRAME_DTYPE.itemsize, 4 * nr if rows else 0
    up = lambda x: (x + 15) & ~15
    f_at = GUARD
    s_at = f_at + up(fb) + GUARD
    r_at = s_at + up(sb) + GUARD
    total = r_at + up(rb) + GUARD
    if device:
        t = torch.full((total,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        base, flags = t.data_ptr(), _lib.DECODE_OUT_DEVICE
    else:
        buf = np.full(total, FILL, dtype=np.uint8)
        base, flags = buf.ctypes.data, 0
    rc = _lib.lib().flacgpu_decoder_analyze(dec._h, flags, base + f_at, nf, base + s_at, ns,
                                            base + r_at if rows else None, nr if rows else 0)
    assert rc == OK, rc
    if device:
        buf = t.cpu().numpy()
    used = np.zeros(total, dtype=bool)
    used[f_at:f_at + fb] = used[s_at:s_at + sb] = True
    used[r_at:r_at + rb] = True
    assert (buf[~used] == FILL).all(), "a write outside the three outputs"
    return gpu.FrameAnalysis(buf[f_at:f_at + fb].view(gpu.ANALYSIS_FRAME_DTYPE).copy(),
                             buf[s_at:s_at + sb].view(gpu.SUBFRAME_DTYPE).copy(),
                             buf[r_at:r_at + rb].view(np.int32).copy() if rows else None)


def check_layout(an):
    """Every frame's records and rows stand at the prefix sums of what the frames in front of it take."""
    sub_at = row_at = 0
    for f in range(an.frames.size):
        fr = an.frames[f]
        assert (int(fr["first_subframe"]), int(fr["row_offset"])) == (sub_at, row_at), f"frame {f} offsets"
        ch, n = int(fr["plan"]["channels"]), int(fr["block_size"])
        sub_at += ch
        row_at += ch * ((n + 3) & ~3)
    assert sub_at == an.subframes.size and (an.rows is None or row_at == an.rows.size)


def check_against_references(an, entries, rows=True):
    """Frame f of the analysis is entries[f]: records and rows against the model, and -- for the oracle's frames --
    through compare_frame against the oracle's plan.  A CONSTANT row is compared at [0] alone."""
    from flac_codec_amd import _lib

    assert an.frames.size == len(entries), f"{an.frames.size} frames analysed, {len(entries)} expected"
    check_layout(an)
    for f, (where, fb, bps, ref) in enumerate(entries):
        m = model_of(fb, bps)
        subs = an.subframes_of(f)
        if m is None:   # a malformed frame: refused, its records and rows unspecified
            assert int(an.frames[f]["status"]) & 1, f"{where}: the model refuses the frame, status {an.frames[f]['status']}"
            continue
        assert int(an.frames[f]["status"]) == 0, f"{where}: status {an.frames[f]['status']}"
        model.assert_records_equal(an.frames[f], subs, m, where)
        if rows:
            model.assert_rows_equal(lambda c: an.row(f, c), m, where)
        if ref is not None and rows:
            plan, planar = ref
            fp = _lib.FramePlan.from_buffer_copy(an.frames[f]["plan"].tobytes())
            sp = [_lib.SubframePlan.from_buffer_copy(s.tobytes()) for s in subs]
            cmp.compare_frame(fp, sp, [an.row(f, c) for c in range(planar.shape[0])], plan, planar, planar.shape[1], where)


def same_records(a, b):
    return a.frames.tobytes() == b.frames.tobytes() and a.subframes.tobytes() == b.subframes.tobytes()


ALL_CASES = lambda: ac.syn_cases() + ac.oracle_cases()


@pytest.mark.parametrize("raw", [False, True], ids=["scan", "scan_frames"])
def test_cases_records_and_rows(dec, raw):
    """Every stream of _analysis_cases in one batch, as .flac files through scan and as bare frames through
    scan_frames: records and rows against the model, the written choices' model and the oracle; the records-only pass
    gives the same records; host output equals device output."""
    cases = ALL_CASES()
    if raw:
        dec.scan_frames([c.raw for c in cases])
    else:
        dec.scan([c.blob for c in cases])
    entries = case_entries(cases)
    an = analyze_guarded(dec, rows=True, device=True)
    check_against_references(an, entries)
    only = analyze_guarded(dec, rows=False, device=True)
    assert same_records(an, only) and only.rows is None
    host = analyze_guarded(dec, rows=True, device=False)
    assert same_records(an, host) and np.array_equal(_defined_rows(an), _defined_rows(host))
    flags = [int(s["reserved"][0]) for s in an.subframes]
    assert any(f & model.AN_WIDE for f in flags) and any(f & model.AN_PARTS_CLIPPED for f in flags)


def _defined_rows(an):
    """The row elements the interface defines, one after another: [0, n) of every row, [0] of a CONSTANT row."""
    out = []
    for f in range(an.frames.size):
        for c, s in enumerate(an.subframes_of(f)):
            r = an.row(f, c)
            out.append(np.asarray(r[:1] if int(s["type"]) == model.SUB_CONSTANT else r))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int32)


def test_python_front_door(dec):
    """gpu.analyze_many and Decoder.analyze: the rows as a CUDA tensor or a numpy array, the same records either way."""
    import torch

    from flac_codec_amd import gpu

    cases = ac.oracle_cases()[:8]
    entries = case_entries(cases)
    a = gpu.analyze_many([c.blob for c in cases], rows=True, out="device", decoder=dec)
    assert isinstance(a.rows, torch.Tensor) and a.rows.is_cuda and a.rows.dtype == torch.int32
    b = gpu.analyze_many([c.raw for c in cases], raw=True, rows=True, out="host")
    assert isinstance(b.rows, np.ndarray)
    check_against_references(b, entries)
    dev = gpu.FrameAnalysis(a.frames, a.subframes, a.rows.cpu().numpy())
    check_against_references(dev, entries)
    c = gpu.analyze_many([c.blob for c in cases], decoder=dec)
    assert c.rows is None and same_records(c, dev)
    with pytest.raises(ValueError):
        gpu.analyze_many([cases[0].blob], speculative=True)


def test_foreign_matrix_permuted(dec):
    """The whole foreign matrix and its malformed streams in one batch, permuted, as .flac files: records and rows
    equal the model, the malformed frames are the ones refused, and per stream as many frames are refused as the
    decoder counts bad."""
    import torch

    from flac_codec_amd import _lib

    streams = list(fmx.valid_cases()) + [s for _, s in fmx.invalid_cases()]
    random.Random(7).shuffle(streams)
    recs, total = dec.scan([s.blob for s in streams])
    entries = []
    for i, st in enumerate(streams):
        assert recs[i].rc == 0 and recs[i].info.frames == st.n_frames, st.name
        entries += [(f"{st.name} frame {k}", fb, st.bps, None) for k, fb in enumerate(st.frame_bytes)]
    an = analyze_guarded(dec, rows=True, device=True)
    check_against_references(an, entries)
    assert max(int(s["partition_order"]) for s in an.subframes) == 15
    only = analyze_guarded(dec, rows=False, device=True)
    assert same_records_where_parsed(an, only)
    pcm = torch.empty(total, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dec.decode(pcm.data_ptr(), total, _lib.DECODE_OUT_DEVICE | _lib.DECODE_NO_MD5, recs)
    f0 = 0
    for i, st in enumerate(streams):
        bad = sum(int(x) & 1 for x in an.frames["status"][f0:f0 + st.n_frames])
        assert bad == recs[i].info.bad_frames == (0 if st.valid else 1), f"{st.name}: {bad} refused, decode counts {recs[i].info.bad_frames}"
        f0 += st.n_frames


def test_status_is_decode_frames_status(dec):
    """Raw frame streams under the speculative scan, in one permuted batch: every stream of _analysis_cases, the
    malformed frames of the matrix written with a sample rate of their own (the matrix's headers leave the rate to the
    STREAMINFO, so a raw scan passes them over), what the raw scan keeps of the matrix itself, and a damaged stream.
    Status bit 0 and bit 1 equal decode_frames' frame by frame; a frame parses exactly when the model parses it; the
    frames that parse give the model's records and rows."""
    import torch

    from flac_codec_amd import _lib

    blobs = [(c.name, c.raw) for c in ALL_CASES() + ac.raw_invalid_cases()]
    blobs += [(s.name, s.blob[len(s.blob) - sum(map(len, s.frame_bytes)):])
              for s in list(fmx.valid_cases()) + [s for _, s in fmx.invalid_cases()]]
    victim = ac.syn_cases()[0]   # eight mono frames
    damaged = bytearray(victim.raw)
    damaged[len(victim.frame_bytes[0]) + 1] ^= 0xFF                   # frame 1: no sync code any more
    damaged[len(damaged) - len(victim.frame_bytes[-1]) // 2] ^= 0x10   # the last frame: a bit of its body
    blobs.append(("damaged", bytes(damaged)))
    random.Random(11).shuffle(blobs)
    _, _, _, frames = dec.scan_frames([b for _, b in blobs], speculative=True)
    expected = sum(len(c.frame_bytes) for c in ALL_CASES() + ac.raw_invalid_cases())
    assert frames.size >= expected + 6, f"{frames.size} frames kept"
    an = analyze_guarded(dec, rows=True, device=True)
    only = analyze_guarded(dec, rows=False, device=True)
    assert same_records_where_parsed(an, only)
    total = dec.raw_elements
    pcm = torch.empty(total, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    decoded = dec.decode_frames(pcm.data_ptr() if total else None, total, _lib.DECODE_OUT_DEVICE, frames.copy())
    check_layout(an)
    assert an.frames.size == frames.size
    n_bad = 0
    for f in range(frames.size):
        rec = decoded[f]
        where = f"{blobs[int(rec['stream'])][0]} at byte {int(rec['byte_offset'])}"
        status = int(an.frames[f]["status"])
        assert status == int(rec["status"]), f"{where}: analysis status {status}, decode_frames {rec['status']}"
        blob = blobs[int(rec["stream"])][1]
        fb = blob[int(rec["byte_offset"]):int(rec["byte_offset"]) + int(rec["bytes"])]
        m = model.parse_frame(fb, 0)
        assert (m is None) == bool(status & 1), f"{where}: status {status}, the model {'refuses' if m is None else 'accepts'}"
        n_bad += status & 1
        if m is not None:
            model.assert_records_equal(an.frames[f], an.subframes_of(f), m, where)
            model.assert_rows_equal(lambda c: an.row(f, c), m, where)
    assert n_bad >= len(fmx.INVALID)


def same_records_where_parsed(a, b):
    if a.frames.tobytes() != b.frames.tobytes():
        return False
    return all(a.subframes_of(f).tobytes() == b.subframes_of(f).tobytes()
               for f in range(a.frames.size) if not int(a.frames[f]["status"]) & 1)


@functools.lru_cache(maxsize=1)
def grid_frames():
    """One-frame raw streams: mono, stereo and 8 channels in turn, at n = 5 and n = 17, FIXED and VERBATIM."""
    rng = random.Random(31)
    out = []
    for i in range(65):
        ch, n = (1, 2, 8)[i % 3], (5, 17)[(i // 3) % 2]
        pcm, subs = [], []
        for c in range(ch):
            sub = fs.fixed((i + c) % 3) if (i + c) % 4 else fs.verbatim()
            v = fmx._predicted(rng, n, 16, sub) if sub["kind"] == "fixed" else [rng.randint(-900, 900) for _ in range(n)]
            pcm.append(v)
            subs.append(fmx.fit_k(v, sub) if sub["kind"] == "fixed" else sub)
        out.append(fs.write_frame(44100, 16, fs.Frame(pcm, subs, number=i, rcode=fs.RATE_CODES[44100]), set()))
    return tuple(out)


@pytest.mark.parametrize("count", [31, 32, 33, 63, 64, 65])
def test_grid_and_offsets(dec, count):
    """Batches around the workgroup (32 lanes) and wave (64) sizes, frames of three shapes in turn: every frame's
    records and rows land at its own first_subframe / row_offset, and nothing outside the outputs is written."""
    frames = grid_frames()[:count]
    dec.scan_frames(list(frames))
    an = analyze_guarded(dec, rows=True, device=True)
    check_against_references(an, [(f"grid frame {i}", fb, 16, None) for i, fb in enumerate(frames)])
    assert [int(x) for x in an.frames["plan"]["channels"][:3]] == [1, 2, 8]


def test_device_input_and_session_feed(dec):
    """Device-resident input and one DecoderSession feed give the records and rows of the one-shot scan of the same bytes."""
    import torch

    from flac_codec_amd.gpu import DecoderSession

    cases = ac.oracle_cases()[4:12] + ac.syn_cases()
    raws = [c.raw for c in cases]
    dec.scan_frames(raws)
    want = analyze_guarded(dec, rows=True, device=True)
    check_against_references(want, case_entries(cases))
    tensors = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in raws]
    dec.scan_frames(tensors)
    got = analyze_guarded(dec, rows=True, device=True)
    assert same_records(got, want) and np.array_equal(_defined_rows(got), _defined_rows(want))
    dec.scan([torch.frombuffer(bytearray(c.blob), dtype=torch.uint8).cuda() for c in cases])
    got = analyze_guarded(dec, rows=True, device=True)
    assert same_records(got, want) and np.array_equal(_defined_rows(got), _defined_rows(want))
    ses = DecoderSession(len(raws), 1 << 16, device=0)
    try:
        frames, _ = ses.feed(raws, flush=True)
        assert frames.size == want.frames.size
        got = ses.decoder.analyze(rows=True, out="host")
        assert same_records(got, want) and np.array_equal(_defined_rows(got), _defined_rows(want))
    finally:
        ses.close()


def test_closed_loop_through_the_packer(dec):
    """decode gives the PCM, analyze the plans, and GpuAnalyzer.pack_plans + fetch_frames give the input frames back byte
    for byte: every frame of every oracle-encoded case (the packer was never promised a foreign plan)."""
    from flac_codec_amd import _lib, gpu

    cases = ac.oracle_cases()
    flat, streams = gpu.decode_many([c.blob for c in cases], out="host", verify_md5=False, decoder=dec)
    an = dec.analyze(rows=False)
    f0 = 0
    for i, case in enumerate(cases):
        nf = len(case.frame_bytes)
        assert streams[i].rc == 0, case.name
        pcm = np.ascontiguousarray(streams[i].pcm, dtype=np.int32)
        assert np.array_equal(pcm.T, np.concatenate(case.planar, axis=1)), f"{case.name}: decoded PCM"
        plans = (_lib.FramePlan * nf)()
        subs = (_lib.SubframePlan * (nf * case.channels))()
        for k in range(nf):
            assert int(an.frames[f0 + k]["status"]) == 0
            plans[k] = _lib.FramePlan.from_buffer_copy(an.frames[f0 + k]["plan"].tobytes())
            for c, s in enumerate(an.subframes_of(f0 + k)):
                subs[k * case.channels + c] = _lib.SubframePlan.from_buffer_copy(s.tobytes())
        o = case.options
        enc = gpu.GpuAnalyzer(o["block_size"], o["max_partition_order"], o["max_lpc_order"], o["mid_side"],
                              o["exhaustive"], 2, 0.5, case.bps, case.channels, max_frames=nf)
        try:
            data, off = enc.pack_plans(pcm, nf, case.sizes[-1], plans, subs, 0, case.rate)
        finally:
            enc.close()
        for k, fb in enumerate(case.frame_bytes):
            assert data[off[k]:off[k + 1]] == fb, f"{case.name} frame {k}: packed bytes differ"
        f0 += nf
    assert f0 == an.frames.size


def test_alternation_with_decode_as(dec):
    """analyze, decode_as, analyze on one scan: the second analysis equals the first, the decode is what it is alone."""
    from flac_codec_amd import _lib
    from flac_codec_amd.gpu import Decoder

    cases = ac.oracle_cases()[:14]
    blobs = [c.blob for c in cases]
    fmt = _lib.OutFormat(_lib.SAMPLE_F32, _lib.LAYOUT_FLAT, 0, 0, 0)

    def decode_as(recs):
        need = Decoder.plan_output(fmt, recs, len(blobs))
        out = np.zeros(need, dtype=np.uint8)
        dec.decode_as(out.ctypes.data, need, fmt, _lib.DECODE_NO_MD5, recs)
        return out

    recs, _ = dec.scan(blobs)
    alone = decode_as(recs)
    recs, _ = dec.scan(blobs)
    first = analyze_guarded(dec, rows=True, device=True)
    between = decode_as(recs)
    second = analyze_guarded(dec, rows=True, device=True)
    assert same_records(first, second) and np.array_equal(_defined_rows(first), _defined_rows(second))
    assert np.array_equal(alone, between) and alone.size
    check_against_references(second, case_entries(cases))


def test_refusals_write_nothing():
    """Before any scan, each cap one short, an unknown flag: the stated rc and not a byte written; a batch without a
    frame succeeds with zero counts."""
    from flac_codec_amd import _lib, gpu

    L = _lib.lib()
    d = gpu.Decoder(0)
    try:
        fsz, ssz = gpu.ANALYSIS_FRAME_DTYPE.itemsize, gpu.SUBFRAME_DTYPE.itemsize
        nf, ns, nr = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
        assert L.flacgpu_decoder_plan_analysis(d._h, C.byref(nf), C.byref(ns), C.byref(nr)) == INVALID_ARG
        assert (nf.value, ns.value, nr.value) == (0, 0, 0)
        cases = ac.oracle_cases()[:6]
        want = (sum(len(c.frame_bytes) for c in cases), sum(len(c.frame_bytes) * c.channels for c in cases),
                sum(c.channels * ((n + 3) & ~3) for c in cases for n in c.sizes))

        def call(flags, f_cap, s_cap, r_cap):
            bufs = [np.full(want[0] * fsz, FILL, dtype=np.uint8), np.full(want[1] * ssz, FILL, dtype=np.uint8),
                    np.full(want[2] * 4, FILL, dtype=np.uint8)]
            rc = L.flacgpu_decoder_analyze(d._h, flags, bufs[0].ctypes.data, f_cap, bufs[1].ctypes.data, s_cap,
                                           bufs[2].ctypes.data, r_cap)
            return rc, all((b == FILL).all() for b in bufs)

        assert call(0, *want) == (INVALID_ARG, True)          # no scanned batch
        d.scan([c.blob for c in cases])
        assert d.plan_analysis() == want
        assert call(0, want[0] - 1, want[1], want[2]) == (TOO_SMALL, True)
        assert call(0, want[0], want[1] - 1, want[2]) == (TOO_SMALL, True)
        assert call(0, want[0], want[1], want[2] - 1) == (TOO_SMALL, True)
        assert call(2, *want) == (INVALID_ARG, True)          # an unknown flag
        assert call(1 | 4, *want) == (INVALID_ARG, True)
        rc, untouched = call(0, *want)
        assert rc == OK and not untouched
        # a batch without a frame: a stream that is metadata alone, and no stream at all
        d.scan([cases[0].blob[:42]])
        assert d.plan_analysis() == (0, 0, 0)
        assert call(0, 0, 0, 0) == (OK, True)
        an = d.analyze(rows=True)
        assert an.frames.size == an.subframes.size == an.rows.size == 0
        d.scan_frames([bytes(10)])   # no frame in it
        assert d.plan_analysis() == (0, 0, 0) and call(0, 0, 0, 0) == (OK, True)
    finally:
        d.close()


def test_frame_iterator_and_the_dump(dec):
    """decode.FrameIterator over .flac files: the reference's names, every value exact -- a 33-bit side channel too --,
    against the model; and the lines examples/flac_analyze.py prints for a frame."""
    import importlib.util
    import os

    from flac_codec_amd import decode

    spec = importlib.util.spec_from_file_location(
        "flac_analyze", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "flac_analyze.py"))
    dump = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump)
    kinds = {model.SUB_CONSTANT: decode.Constant, model.SUB_VERBATIM: decode.Verbatim, model.SUB_FIXED: decode.Fixed,
             model.SUB_LPC: decode.Lpc}
    seen = set()
    for case in ac.syn_cases()[:3] + tuple(c for c in ac.oracle_cases() if c.name in ("stereo left/side", "a click in silence")):
        got = list(decode.FrameIterator(case.blob))
        assert len(got) == len(case.frame_bytes), case.name
        at = len(case.blob) - len(case.raw)
        for k, ((frame, offset), fb) in enumerate(zip(got, case.frame_bytes)):
            m, where = model_of(fb, case.bps), f"{case.name} frame {k}"
            assert (offset, frame.bits, frame.status) == (at, 8 * len(fb), 0), where
            at += len(fb)
            h = frame.header
            assert (h.block_size, h.channels, h.sample_rate, h.bits_per_sample) == (m.n, m.channels, case.rate, case.bps), where
            assert h.channel_assignment == {8: "LEFT_SIDE", 9: "SIDE_RIGHT", 10: "MID_SIDE"}.get(m.acode, "INDEPENDENT")
            if hasattr(case, "frames"):
                assert (h.frame_number, h.blocking_strategy) == (case.frames[k].number, bool(case.frames[k].blocking)), where
            for c, (s, ms) in enumerate(zip(frame.subframes, m.subs)):
                assert type(s) is kinds[ms.type] and s.wasted_bps == ms.wasted and s.wide == bool(ms.flags & model.AN_WIDE), where
                row = m.rows[c]
                if ms.type == model.SUB_CONSTANT:
                    assert (s.sample, s.block_size) == (row[0], m.n), where
                elif ms.type == model.SUB_VERBATIM:
                    assert [int(v) for v in s.samples] == row, where
                else:
                    assert s.order == ms.order and [int(v) for v in s.warm_up] == row[:ms.order], where
                    if ms.type == model.SUB_LPC:
                        assert (s.precision, s.shift, s.coefficients) == (ms.precision, ms.shift, ms.coeffs[:ms.order]), where
                    r = s.residuals
                    assert (r.coding_method(), r.partition_order()) == (("RICE", "RICE2")[ms.coding_method], ms.partition_order)
                    assert r.clipped == bool(ms.flags & model.AN_PARTS_CLIPPED) and len(r.partitions) == min(ms.n_partitions, 64)
                    i = ms.order
                    for p, prm in zip(r.partitions, ms.all_params):
                        seen.add(type(p).__name__)
                        if isinstance(p, decode.Standard):
                            assert p.rice == prm, where
                        elif isinstance(p, decode.Escaped):
                            assert ("escape", p.escape_size) == prm and p.escape_size, where
                        else:
                            assert prm == ("escape", 0), where
                        assert [int(v) for v in p.residuals] == row[i:i + len(p.residuals)], where
                        i += len(p.residuals)
                seen.add((type(s).__name__, s.wide))
            lines = list(dump.frame_lines(frame, offset))
            assert lines[0].startswith(f"frame={h.frame_number}\toffset={offset}\tbits={8 * len(fb)}\tblocksize={m.n}\t")
            assert sum(1 for x in lines if x.startswith("\tsubframe=")) == m.channels
            assert sum(1 for x in lines if x.startswith("\t\tparameter[")) == sum(min(s.n_partitions, 64) for s in m.subs)
    assert {"Standard", "Escaped", "ConstantPartition", ("Lpc", True), ("Fixed", True), ("Verbatim", True),
            ("Constant", True), ("Lpc", False)} <= seen, seen
