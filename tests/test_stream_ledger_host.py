"""StreamLedger (csrc/host/stream_ledger.h): the container state of one stream -- open, admit, frames, overrun, close and the
totals verdict -- through tests/stream_ledger_main.cpp, a stand-alone program built from host/stream_ledger.cpp ALONE with
ASan and UBSan.  That it links without the rest of the host driver and without HIP is itself the check that the unit has no
GPU dependency.  CPU only; nothing is loaded into Python under a sanitizer.

Expected header bytes are the head of the oracle's files (oracle_file of test_stream_header_unknown_total.py); the clamp is
checked against Encoder::encode's rule restated below (oracle/flac_oracle.c encoder_encode)."""
import hashlib
import os
import shutil
import subprocess

import pytest

from test_stream_header_unknown_total import BPS, CH, OPTION_SETS, RATE, _le, options_of, oracle_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flac-codec_amd", "csrc", "host")
EXCESSIVE_TOTAL_SAMPLES, SAMPLE_COUNT_MISMATCH, NO_SAMPLES = -116, -117, -118
MAX_SAMPLES = 1 << 36             # Encoder::MAX_SAMPLES
MAX_FRAME_SIZE = (1 << 24) - 1    # Streaminfo::MAX_FRAME_SIZE

STREAMS = [(4096, 9 * 4096 + 100), (1152, 30 * 1152)]   # (block, samples per channel): a short last block; whole blocks only


@pytest.fixture(scope="module")
def ledger_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stream_ledger")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    (tmp / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + san + [str(tmp / "empty.cpp"), "-o", str(tmp / "empty")], capture_output=True, text=True)
    if probe.returncode:
        pytest.skip("the sanitizer runtime cannot be linked here: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    exe = tmp / "stream_ledger_main"
    made = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + [
        "-I" + HOST, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stream_ledger_main.cpp"),
        os.path.join(HOST, "stream_ledger.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr

    def run(cases):
        path = tmp / "cases.txt"
        path.write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
        done = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        lines = done.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines

    return run


def _hex(s):
    return "-" if s is None else s.hex()


def header_case(block, n, name, total_known, cuts):
    pcm, ref, first, sizes = oracle_file(block, n, name, total_known)
    assert sum(cuts) == len(sizes)
    co = options_of(block, name)._c_options()
    tags = [co.comment_fields[i] for i in range(co.n_comment_fields)]
    case = ["header", block, RATE, BPS, CH, int(total_known), n if total_known else 0, co.padding, co.seektable_mode,
            co.seektable_value, _hex(co.vendor_string), len(tags)] + [_hex(t) for t in tags]
    case += [hashlib.md5(_le(pcm, BPS)).hexdigest(), n - (len(sizes) - 1) * block, len(cuts)] + list(cuts) + sizes
    return case, ref[:first]


@pytest.mark.parametrize("total_known", [False, True])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_batch_cuts_give_the_oracles_header(ledger_exe, name, total_known):
    """frames() accumulates across runs: however a stream's frames are cut into batches, close() leaves the oracle's bytes"""
    cases, want = [], []
    for block, n in STREAMS:
        frames = (n + block - 1) // block
        for cuts in ([frames], [1] * frames, [1, 2, frames - 3]):
            case, head = header_case(block, n, name, total_known, cuts)
            cases.append(case)
            want.append(head)
    for case, head, line in zip(cases, want, ledger_exe(cases)):
        rc, got = line.split()
        assert rc == "0", case[:12]
        assert bytes.fromhex(got) == head, case[:12]


def encode_rule(total, written, seek_points, n_frames, last_len, block):
    """Encoder::encode, frame by frame (oracle/flac_oracle.c encoder_encode): the seek point and the sample count first, then
    the error, then the frame.  -> (frames encoded, error, samples_written, seek points)"""
    for f in range(n_frames):
        seek_points += 1
        written += last_len if f + 1 == n_frames else block
        if total and written > total:
            return f, EXCESSIVE_TOTAL_SAMPLES, written, seek_points
    return n_frames, 0, written, seek_points


ADMIT_RUNS = {
    "first_frame": [(5, 16), (2, 16)],            # the total's whole blocks, then a run whose first block is too many
    "mid_batch": [(3, 16), (4, 16)],
    "short_last_frame_one_too_long": [(6, 4)],
    "ends_on_the_total": [(2, 16), (4, 3)],
}


def test_admit_and_overrun_against_the_encode_rule(ledger_exe):
    block, total = 16, 5 * 16 + 3
    names = list(ADMIT_RUNS)
    lines = ledger_exe([["admit", block, total, len(ADMIT_RUNS[k])] + [v for run in ADMIT_RUNS[k] for v in run] for k in names])
    seen = {}
    for name, line in zip(names, lines):
        written = seek_points = 0
        for (n_frames, last_len), got in zip(ADMIT_RUNS[name], line.split("|")):
            usable, err, written, seek_points = encode_rule(total, written, seek_points, n_frames, last_len, block)
            assert [int(v) for v in got.split()] == [usable, err, 0, written, seek_points], (name, line)
        seen[name] = (usable, err)
    assert seen == {"first_frame": (0, EXCESSIVE_TOTAL_SAMPLES), "mid_batch": (2, EXCESSIVE_TOTAL_SAMPLES),
                    "short_last_frame_one_too_long": (5, EXCESSIVE_TOTAL_SAMPLES), "ends_on_the_total": (4, 0)}


def test_totals_verdict(ledger_exe):
    cases = [(1, 83, 83), (1, 83, 80), (0, 0, 0), (0, 0, MAX_SAMPLES), (0, 0, MAX_SAMPLES - 1), (1, 83, 84)]
    got = [int(v) for v in ledger_exe([["verdict"] + list(c) for c in cases])]
    assert got == [0, SAMPLE_COUNT_MISMATCH, NO_SAMPLES, EXCESSIVE_TOTAL_SAMPLES, 0, SAMPLE_COUNT_MISMATCH]


def test_frame_size_rule(ledger_exe):
    """a frame of 0 bytes, or of MAX_FRAME_SIZE and more, leaves STREAMINFO's minimum and maximum alone"""
    got = ledger_exe([["sizes", 0, MAX_FRAME_SIZE], ["sizes", MAX_FRAME_SIZE - 1],
                      ["sizes", 100, 0, MAX_FRAME_SIZE, 50, MAX_FRAME_SIZE - 1, MAX_FRAME_SIZE + 1]])
    assert [tuple(int(v) for v in g.split()) for g in got] == [(0, 0), (MAX_FRAME_SIZE - 1, MAX_FRAME_SIZE - 1),
                                                               (50, MAX_FRAME_SIZE - 1)]
