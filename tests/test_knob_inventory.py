"""Every FLACGPU_* selector that read_knobs() reads is exercised by something and documented.

A selector that keeps a kernel or a path reachable and that nothing sets is code that is compiled,
shipped and never run.  So: each "FLACGPU_..." string literal in the body of read_knobs()
(flac-codec_amd/csrc/flacenc_gpu.hip), other than FLACGPU_TEST_KNOBS itself, must be named by
another file under tests/, by a file under tools/ or by bench.py, and must have a row in the table
of DESIGN.md."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "flac-codec_amd", "csrc", "flacenc_gpu.hip")


def read_knobs_body(text):
    """The text between the braces of `Knobs read_knobs() { ... }`."""
    start = text.index("Knobs read_knobs() {")
    i = text.index("{", start)
    depth = 0
    for j in range(i, len(text)):
        if text[j] == "{":
            depth += 1
        elif text[j] == "}":
            depth -= 1
            if depth == 0:
                return text[i + 1:j]
    raise AssertionError("read_knobs(): unbalanced braces")


def selectors(path=SOURCE):
    with open(path) as f:
        body = read_knobs_body(f.read())
    names = sorted(set(re.findall(r'"(FLACGPU_[A-Z0-9_]+)"', body)))
    assert "FLACGPU_TEST_KNOBS" in names and len(names) > 5, names
    return [n for n in names if n != "FLACGPU_TEST_KNOBS"]


def users():
    """path -> text of every file that may exercise a selector."""
    me = os.path.abspath(__file__)
    out = {}
    for top in ("tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "bin", "golden")]
            for name in files:
                p = os.path.join(d, name)
                if os.path.abspath(p) == me or name.endswith((".pyc", ".so", ".o")):
                    continue
                with open(p, errors="replace") as f:
                    out[os.path.relpath(p, ROOT)] = f.read()
    with open(os.path.join(ROOT, "bench.py")) as f:
        out["bench.py"] = f.read()
    return out


def documented_rows():
    """Selector names in the first column of DESIGN.md's table rows."""
    rows = set()
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        for line in f:
            if line.startswith("| `FLACGPU_"):
                rows.update(re.findall(r"`(FLACGPU_[A-Z0-9_]+)`", line.split("|")[1]))
    return rows


def unexercised(names, texts):
    return [n for n in names if not any(re.search(r"\b%s\b" % n, t) for t in texts.values())]


def test_every_selector_is_exercised_and_documented():
    names = selectors()
    missing = unexercised(names, users())
    assert not missing, "read_knobs() reads selectors that no test, tool or bench leg names: %s" % missing
    undocumented = [n for n in names if n not in documented_rows()]
    assert not undocumented, "selectors without a row in DESIGN.md's table: %s" % undocumented
