"""bench.py --dump-outputs on a plain run (no --full): the frames of the LAST timed step -- the batch of the context the
rotation ends on -- written as float arrays, the oracle's frames of that context's input, and the same arrays whatever the
length of the time-based pre-warm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 24


def _run(tmp_path, name, prewarm_ms):
    d = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(FRAMES), "--steps", "3",
                        "--warmup", "2", "--prewarm-ms", str(prewarm_ms), "--contexts", "2", "--dump-outputs", str(d)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {n: np.load(d / f"{n}.npy") for n in ("frame_offsets", "frame_index", "frame_bytes")}


def test_plain_run_dumps_the_last_steps_frames(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import _oracle as orc
    from _compare import orc_options_for

    line, a = _run(tmp_path, "a", 0)
    assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["roofline"] is None and line["cpu_baseline"] is None and "bit-exact" in line["metric"]
    assert abs(line["value"] - FRAMES * 4096 * 2 / (line["ms_per_step"] * 1e-3) / 1e6) / line["value"] < 1e-2
    off, body = a["frame_offsets"], a["frame_bytes"]
    assert off.dtype == np.float64 and off.shape == (FRAMES + 1,) and off[0] == 0
    assert a["frame_index"].tolist() == list(range(FRAMES))
    assert body.dtype == np.float32 and body.size == off[-1]
    # the pre-warm ends on a whole rotation; 2 warm-up + 3 timed steps over 2 contexts: the last step is context 0's
    cfg = bench.CONFIGS[3]
    pcm = bench.make_pcm(1000 + 16 * 3, FRAMES, cfg["ch"], cfg["bps"])
    oopts = orc_options_for(bench.BLOCK, cfg["po"], cfg["lpc"], True, True)
    raw = body.astype(np.uint8).tobytes()
    per = bench.BLOCK * cfg["ch"]
    for f in range(FRAMES):
        planar = np.ascontiguousarray(pcm[f * per:(f + 1) * per].reshape(bench.BLOCK, cfg["ch"]).T)
        rc, fb, _ = orc.encode_frame(oopts, cfg["rate"], cfg["bps"], planar, frame_number=f)
        assert rc == 0 and raw[int(off[f]):int(off[f + 1])] == fb, f"frame {f} differs from the oracle"
    _, b = _run(tmp_path, "b", 200)          # another pre-warm length: another number of untimed steps
    for k in a:
        assert np.array_equal(a[k], b[k]), k
