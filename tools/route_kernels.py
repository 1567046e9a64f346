"""Which kernels a batch runs, case by case: the per-kernel timing slots (flacgpu_get_kernel_ms) that are non-zero
after an analysis and a frame assembly, and whether the candidate kernel hands its residuals over (handed_subframes).

    python tools/route_kernels.py [out.json]       (default: tests/golden/route_kernels.json)

Uses nothing but GpuAnalyzer's long-standing calls, so it runs on any commit: the committed file is recorded BEFORE a
change to the dispatcher and tests/test_gpu_route_kernels.py holds the changed library to it.  Every case is a batch
of 3 frames (a first, a middle and a last one) and must also decode back to its input (verify_device)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FRAMES = 3
RATE = 48000
KNOB_NAMES = ("FLACGPU_NO_DIRECT", "FLACGPU_NO_W64", "FLACGPU_NO_FUSED_PACK", "FLACGPU_NO_FRAME64", "FLACGPU_NO_HAND",
              "FLACGPU_NO_XPOSE", "FLACGPU_NO_DIRECT_SHORT")


def case(name, channels=2, bps=24, block=4096, order=12, exhaustive=True, last_len=None, layout=0, offset=0,
         packed=0, env=()):
    return dict(name=name, channels=channels, bps=bps, block=block, order=order, exhaustive=exhaustive,
                last_len=last_len or block, layout=layout, offset=offset, packed=packed, env=tuple(env))


CASES = [
    case("stereo"),
    case("stereo_order32", order=32),
    case("stereo_order0", order=0),
    case("stereo_fast_choice", exhaustive=False),
    case("stereo_1152_order8", block=1152, order=8),
    case("stereo_1152_order8_no_direct_short", block=1152, order=8, env=("FLACGPU_NO_DIRECT_SHORT",)),
    case("stereo_4608", block=4608),
    case("stereo_last1000", last_len=1000),
    case("stereo_32bit", bps=32),
    case("stereo_offset4", offset=1),
    case("stereo_planar", layout=1),
    case("stereo_packed3", packed=3),
    case("mono", channels=1),
    case("ch3", channels=3),
    case("ch4", channels=4),
    case("ch5", channels=5),
    case("ch6", channels=6),
    case("ch8", channels=8),
    case("ch4_no_xpose", channels=4, env=("FLACGPU_NO_XPOSE",)),
    case("ch8_order32", channels=8, order=32),
    case("stereo_no_direct", env=("FLACGPU_NO_DIRECT",)),
    case("stereo_no_w64", env=("FLACGPU_NO_W64",)),
    case("stereo_no_fused_pack", env=("FLACGPU_NO_FUSED_PACK",)),
    case("stereo_no_frame64", env=("FLACGPU_NO_FRAME64",)),
    case("stereo_no_hand", env=("FLACGPU_NO_HAND",)),
]


def make_pcm(c, seed):
    """Interleaved int32 samples of the case's batch: a slow sine per channel plus noise, an eighth of full scale."""
    n = (N_FRAMES - 1) * c["block"] + c["last_len"]
    rng = np.random.Generator(np.random.PCG64(seed))
    amp = float(1 << (c["bps"] - 4))
    t = np.arange(n, dtype=np.float64)[:, None]
    ch = np.arange(c["channels"], dtype=np.float64)[None, :]
    x = amp * np.sin(t * (0.01 + 0.003 * ch)) + rng.uniform(-amp / 64, amp / 64, size=(n, c["channels"]))
    return np.ascontiguousarray(np.rint(x).astype(np.int64).astype(np.int32).reshape(-1))


def to_planar(pcm, c):
    """[frame][channel][sample] of whole blocks (the device layout FLACGPU_LAYOUT_PLANAR)."""
    assert c["last_len"] == c["block"]
    return np.ascontiguousarray(pcm.reshape(N_FRAMES, c["block"], c["channels"]).transpose(0, 2, 1).reshape(-1))


def run_case(c, seed=7700):
    """{'kernels': sorted names of the timing slots that ran, 'hand': hand-over enabled, 'verified': decodes back}."""
    import torch

    from flac_codec_amd.gpu import GpuAnalyzer

    saved = {k: os.environ.pop(k, None) for k in KNOB_NAMES}
    for k in c["env"]:
        os.environ[k] = "1"
    try:
        an = GpuAnalyzer(c["block"], 6, c["order"], True, c["exhaustive"], 2, 0.5, c["bps"], c["channels"],
                         max_frames=N_FRAMES)
    finally:
        for k in c["env"]:
            del os.environ[k]
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    try:
        an.set_timing(True)
        pcm = make_pcm(c, seed)
        if c["packed"]:
            le = pcm.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :c["packed"]]
            an.encode_packed(np.ascontiguousarray(le).reshape(-1), c["packed"], N_FRAMES, c["last_len"], 0, RATE)
        else:
            src = to_planar(pcm, c) if c["layout"] == 1 else pcm
            dev = torch.zeros(src.size + 64 + c["offset"], dtype=torch.int32, device="cuda")
            dev[c["offset"]:c["offset"] + src.size] = torch.from_numpy(src).cuda()
            torch.cuda.synchronize()
            an.analyze_device(dev.data_ptr() + 4 * c["offset"], N_FRAMES, c["last_len"], layout=c["layout"])
            an.pack_device(0, RATE)
        kernels = sorted(an.kernel_ms())
        hand = an.handed_subframes()[2]
        res, _ = an.verify_device(RATE, 0)
        verified = (res.frames, res.bad_structure, res.bad_crc16, res.frames_pcm_differs, res.samples_differ) == \
            (N_FRAMES, 0, 0, 0, 0) and bool(res.compared_pcm)
    finally:
        an.close()
    return {"kernels": kernels, "hand": bool(hand), "verified": bool(verified)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "route_kernels.json")
    table = {}
    for c in CASES:
        table[c["name"]] = run_case(c)
        print(c["name"], table[c["name"]], flush=True)
        if not table[c["name"]]["verified"]:
            raise SystemExit("case %s does not decode back to its input" % c["name"])
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
