"""Frame analysis on the host: the rule of csrc/kernels/frame_analysis.h (flacgpu_analyze_frame_host) against a plain
Python restatement (_frame_model) that has two references of its own -- the choices _flacsyn wrote, and the oracle's
plans -- and against the oracle directly.  No device."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _analysis_cases as ac
import _compare as cmp
import _foreign_matrix as fmx
import _frame_model as model
from flac_codec_amd import _lib, gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_frames():
    """(where, frame bytes, STREAMINFO sample size) of every frame of the cases and of the foreign matrix."""
    for case in ac.syn_cases() + ac.oracle_cases():
        for k, fb in enumerate(case.frame_bytes):
            yield f"{case.name} frame {k}", fb, case.bps
    for st in fmx.valid_cases():
        for k, fb in enumerate(st.frame_bytes):
            yield f"{st.name} frame {k}", fb, st.bps


def test_model_returns_the_written_choices():
    n = 0
    for case in ac.syn_cases():
        for k, (fb, fr) in enumerate(zip(case.frame_bytes, case.frames)):
            ac.check_choices(model.parse_frame(fb, case.bps), fr, f"{case.name} frame {k}")
            n += 1
    assert n >= 20
    flags = [s.flags for case in ac.syn_cases() for fb in case.frame_bytes for s in model.parse_frame(fb, case.bps).subs]
    assert any(f & model.AN_PARTS_CLIPPED for f in flags) and any(f & model.AN_WIDE for f in flags)


def test_model_passes_compare_frame_on_the_oracles_frames():
    for case in ac.oracle_cases():
        for k, (fb, plan, planar) in enumerate(zip(case.frame_bytes, case.plans, case.planar)):
            m = model.parse_frame(fb, case.bps)
            assert m is not None and m.crc_ok, f"{case.name} frame {k}"
            rows = [np.array(r, dtype=np.int64).astype(np.int32) for r in m.rows]
            cmp.compare_frame(m, m.subs, rows, plan, planar, planar.shape[1], f"{case.name} frame {k}")


def test_host_rule_equals_the_model_on_every_frame():
    n = 0
    for where, fb, bps in all_frames():
        m = model.parse_frame(fb, bps)
        assert m is not None, where
        fa, subs, rows = gpu.analyze_frame_host(fb, bps)
        assert int(fa["status"]) == 0, f"{where} status {fa['status']}"
        assert int(fa["row_offset"]) == 0 and int(fa["first_subframe"]) == 0
        model.assert_records_equal(fa, subs, m, where)
        model.assert_rows_equal(lambda c: rows[c], m, where, wide_low32=False)   # int64 rows: a wide subframe is exact
        fa2, subs2, _ = gpu.analyze_frame_host(fb, bps, rows=False)
        assert fa2.tobytes() == fa.tobytes() and subs2.tobytes() == subs.tobytes(), f"{where} records-only pass"
        n += 1
    assert n > 300   # nothing was skipped


def test_host_rule_passes_compare_frame_on_the_oracles_frames():
    for case in ac.oracle_cases():
        for k, (fb, plan, planar) in enumerate(zip(case.frame_bytes, case.plans, case.planar)):
            fa, subs, rows = gpu.analyze_frame_host(fb, case.bps)
            assert int(fa["status"]) == 0
            fp = _lib.FramePlan.from_buffer_copy(fa["plan"].tobytes())
            sp = [_lib.SubframePlan.from_buffer_copy(s.tobytes()) for s in subs]
            cmp.compare_frame(fp, sp, rows.astype(np.int32), plan, planar, planar.shape[1], f"{case.name} frame {k}")


def test_a_sample_size_left_to_the_streaminfo():
    """A header with sample-size code 0 is analysed with the STREAMINFO's size, and refused without one."""
    st = next(s for s in fmx.valid_cases() if ("bps_code", 0) in s.features)
    hits = 0
    for fb in st.frame_bytes:
        if (fb[3] >> 1) & 7:
            continue
        hits += 1
        assert int(gpu.analyze_frame_host(fb, st.bps)[0]["status"]) == 0
        assert int(gpu.analyze_frame_host(fb, 0)[0]["status"]) & 1
        assert model.parse_frame(fb, 0) is None
    assert hits


def _guarded_call(fb, bps, rows_elems):
    """flacgpu_analyze_frame_host into buffers with guard regions; returns (rc, status, guards intact)."""
    G = 64
    fa = np.full(G + C.sizeof(_lib.FrameAnalysis) + G, 0xA5, dtype=np.uint8)
    subs = np.full(G + 8 * C.sizeof(_lib.SubframePlan) + G, 0xA5, dtype=np.uint8)
    rows = np.full(G // 8 + rows_elems + G // 8, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    rc = _lib.lib().flacgpu_analyze_frame_host(
        fb, len(fb), bps, C.cast(fa.ctypes.data + G, C.POINTER(_lib.FrameAnalysis)),
        C.cast(subs.ctypes.data + G, C.POINTER(_lib.SubframePlan)), rows.ctypes.data + G, rows_elems)
    intact = (np.all(fa[:G] == 0xA5) and np.all(fa[-G:] == 0xA5) and np.all(subs[:G] == 0xA5)
              and np.all(subs[-G:] == 0xA5) and np.all(rows[:G // 8] == 0x5A5A5A5A5A5A5A5A)
              and np.all(rows[-(G // 8):] == 0x5A5A5A5A5A5A5A5A))
    status = int(np.frombuffer(fa[G:G + C.sizeof(_lib.FrameAnalysis)].tobytes(), dtype=gpu.ANALYSIS_FRAME_DTYPE)[0]["status"])
    return rc, status, bool(intact), rows


def test_malformed_frames_are_refused_as_the_model_refuses_them():
    for reason, st in fmx.invalid_cases():
        refused = []
        for k, fb in enumerate(st.frame_bytes):
            m = model.parse_frame(fb, st.bps)
            n = st.frame_sizes[k]
            rc, status, intact, _ = _guarded_call(fb, st.bps, (n + 3) & ~3)
            assert rc == 0 and intact, f"{reason} frame {k}: rc {rc}, guards intact {intact}"
            assert (status & 1) == (m is None), f"{reason} frame {k}: status {status}, model {'refuses' if m is None else 'accepts'}"
            assert status & 2 == 0   # _flacsyn writes a right CRC-16 over what it wrote
            refused.append(m is None)
        assert refused == [False, True, False], reason


def test_rows_that_do_not_fit_are_refused_and_nothing_is_written():
    case = ac.oracle_cases()[6]   # n = 192, mono
    fb = case.frame_bytes[0]
    rc, _, intact, rows = _guarded_call(fb, case.bps, 191)
    assert rc == -5 and intact and np.all(rows == 0x5A5A5A5A5A5A5A5A)
    damaged = fb[:-2] + bytes([fb[-2] ^ 1, fb[-1]])
    assert int(gpu.analyze_frame_host(damaged, case.bps)[0]["status"]) == 2   # parses; the CRC-16 is wrong


def test_host_rule_under_the_sanitizers(tmp_path):
    """Every truncation and 300 single-bit flips of six frames through a stand-alone program built with
    -fsanitize=address,undefined: no report, exit status 0.  Nothing is loaded into Python under a sanitizer."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(REPO, "flac-codec_amd", "csrc")
    srcs = [os.path.join(REPO, "tests", "frame_analysis_fuzz_main.cpp")] + [
        os.path.join(csrc, "host", f) for f in ("frame_analysis.cpp", "flac_stream.cpp", "checksums.cpp")]
    exe = str(tmp_path / "frame_analysis_fuzz")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"), "-I", os.path.join(csrc, "host"),
            "-o", exe] + srcs
    # the runtimes inside the program where the toolchain has them as archives, else the shared ones
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode:
        build = subprocess.run(base, capture_output=True, text=True)
    if build.returncode and ("asan" in build.stderr or "ubsan" in build.stderr) and "cannot find" in build.stderr:
        pytest.skip("the sanitizer runtime does not link here")
    assert build.returncode == 0, build.stderr[-2000:]
    syn = {c.name: c for c in ac.syn_cases()}
    orc_ = {c.name: c for c in ac.oracle_cases()}
    picks = [(syn["syn-kinds"], 5), (syn["syn-kinds"], 7), (syn["syn-clipped"], 0), (syn["syn-wide-a"], 4),
             (orc_["8 channels"], 0), (orc_["a click in silence"], 0)]
    blob = b"".join(struct.pack("<II", len(c.frame_bytes[k]), c.bps) + c.frame_bytes[k] for c, k in picks)
    path = tmp_path / "frames.bin"
    path.write_bytes(blob)
    run = subprocess.run([exe, str(path), "300"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-500:]}\n{run.stderr[-3000:]}"
    assert "damaged frames analysed" in run.stdout
