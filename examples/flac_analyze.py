#!/usr/bin/env python3
"""flac_analyze.py FILE.flac [FILE.flac ...]

A full analysis dump of FLAC files, like the reference implementation's `flac -a` and the reference crate's
examples/flac-analyze.rs: one line per frame, one per subframe, then the predictor's coefficients, the warm-up samples
and every residual partition's parameter.  The residuals themselves are left out.  Every frame of every file is
analysed in one GPU batch per file (flac_codec_amd.decode.FrameIterator over gpu.analyze_many); with several files the
dumps follow one another under a `file=` line."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from flac_codec_amd.decode import (ConstantPartition, Escaped, FrameIterator, Standard)   # noqa: E402


def residual_lines(residuals):
    for num, p in enumerate(residuals.partitions):
        if isinstance(p, Standard):
            yield "\t\tparameter[%d]=%d" % (num, p.rice)
        elif isinstance(p, Escaped):
            yield "\t\tparameter[%d]=ESCAPE, raw_bits=%d" % (num, p.escape_size)
        elif isinstance(p, ConstantPartition):
            yield "\t\tparameter[%d]=ESCAPE, raw_bits=0" % num


def subframe_lines(num, s):
    head = "\tsubframe=%d\twasted_bits=%d\ttype=%s" % (num, s.wasted_bps, s.subframe_type())
    kind = s.subframe_type()
    if kind == "CONSTANT":
        yield head + "\tvalue=%d" % s.sample
        return
    if kind == "VERBATIM":
        yield head
        return
    head += "\torder=%d" % s.order
    if kind == "LPC":
        head += "\tqlp_coeff_precision=%d\tquantization_level=%d" % (s.precision, s.shift)
    yield head + "\tresiduals_type=%s\tpartition_order=%d" % (s.residuals.coding_method(), s.residuals.partition_order())
    if kind == "LPC":
        for k, c in enumerate(s.coefficients):
            yield "\t\tqlp_coeff[%d]=%d" % (k, c)
    for k, w in enumerate(s.warm_up):
        yield "\t\twarmup[%d]=%d" % (k, int(w))
    yield from residual_lines(s.residuals)


def frame_lines(frame, offset):
    h = frame.header
    yield "frame=%d\toffset=%d\tbits=%d\tblocksize=%d\tsample_rate=%d\tchannels=%d\tchannel_assignment=%s" % (
        h.frame_number, offset, frame.bits, h.block_size, h.sample_rate, h.channels, h.channel_assignment)
    if frame.status & 1:
        yield "\t* the frame does not parse"
    for num, s in enumerate(frame.subframes):
        yield from subframe_lines(num, s)


def main(argv):
    if len(argv) < 2:
        print("* Usage: flac_analyze.py <file.flac> [...]", file=sys.stderr)
        return 2
    for path in argv[1:]:
        if len(argv) > 2:
            print("file=%s" % path)
        try:
            with open(path, "rb") as f:
                data = f.read()
            for frame, offset in FrameIterator(data):
                print("\n".join(frame_lines(frame, offset)))
        except Exception as e:   # one bad file does not hide the others
            print("* %s, %s" % (path, e), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
