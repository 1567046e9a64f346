"""The decoder-session rule (DESIGN.md 4b "Decoder sessions") as _session_model.py states it, held to itself -- online()
feed by feed against segments() over the whole bytes -- and to the raw rule of _raw_frames.py.  No library, no GPU."""
import random

import pytest

import _raw_frames as rf
import _session_model as sm

W = 1024   # holds every frame of the two streams (the model confirms it: raw_links_within)


def _same(blob, cuts, flushes, w, label):
    feeds, summary, held = sm.online(blob, cuts, flushes, w)
    want, want_summary = sm.segments(blob, flushes, w)
    got = [r for f in feeds for r in f]
    assert sm.tuples(got) == sm.tuples(want), label
    assert summary == want_summary, label
    assert held <= w + 15, label
    return feeds


@pytest.mark.parametrize("which", ["uniform", "mixed"])
def test_every_single_cut(which):
    st = rf.uniform() if which == "uniform" else rf.mixed()
    whole, _ = sm.segments(st.blob, (), W)
    assert sm.tuples(whole) == sm.tuples([dict(r, out_offset=0) for r in rf.expected_records(st)])
    assert sm.raw_links_within(st.blob, W)
    for cut in range(1, len(st.blob)):
        feeds = _same(st.blob, [cut, len(st.blob)], set(), W, f"{which}: cut at {cut}")
        assert sm.tuples([r for f in feeds for r in f]) == sm.tuples(whole)   # the cut does not matter


def test_the_twelve_frame_stream_is_the_one_of_raw_frames():
    assert len(rf.mixed().blob) == 2105 and len(rf.mixed().frame_bytes) == 12


def test_seeded_multi_cuts_with_flushes():
    rng = random.Random(20261023)
    flushed_wrong = 0
    for k in range(200):
        st = rf.mixed() if k & 1 else rf.uniform()
        cuts, flushes = sm.multi_cut(rng, st)
        _same(st.blob, cuts, flushes, W, f"case {k}")
        flushed_wrong += any(f not in st.at for f in flushes)
    assert flushed_wrong > 20   # the wrong places are really among the cases


def test_without_flush_and_a_wide_bound_the_rule_is_the_raw_rule():
    for label, blob in rf.all_cases()[::37] + rf.all_cases()[:3]:
        records, (frames, skipped, gaps) = sm.segments(blob, (), max(len(blob), 16))
        want, summary = rf.scan(blob)
        assert sm.tuples(records) == sm.tuples([dict(r, out_offset=0) for r in want]), label
        assert (frames, skipped, gaps) == (summary["frames"], summary["skipped_bytes"], summary["gaps"]), label
        assert sm.raw_links_within(blob, max(len(blob), 16)), label


def test_an_end_exactly_W_away_is_kept_and_one_byte_further_is_passed_over():
    st = rf.uniform()
    longest = max(len(c) for c in st.frame_bytes)
    k = [len(c) for c in st.frame_bytes].index(longest)
    kept, _ = sm.segments(st.blob, (), longest)
    assert len(kept) == len(st.frame_bytes)
    lost, (frames, skipped, gaps) = sm.segments(st.blob, (), longest - 1)
    assert st.at[k] not in [r["byte_offset"] for r in lost] and frames < len(st.frame_bytes) and skipped >= longest
    assert not sm.raw_links_within(st.blob, longest - 1) and sm.raw_links_within(st.blob, longest)
    for w in (longest, longest - 1):   # and feed by feed
        rng = random.Random(w)
        for _ in range(20):
            cuts, flushes = sm.multi_cut(rng, st, flush_rate=0)
            _same(st.blob, cuts, flushes, w, f"W = {w}")


def test_a_candidate_at_L_minus_16_is_judged_and_at_L_minus_15_held():
    st = rf.uniform()
    two = st.at[2]   # frames 0 and 1, then the header of frame 2
    for extra, decided in ((16, 2), (15, 1)):
        s = sm.Online(W)
        got = s.feed(st.blob[:two + extra])
        # frame 1 ends at frame 2's header, which is a candidate once 16 bytes follow it
        assert len(got) == decided, extra
        assert len(s.tail) == (16 if extra == 16 else 15 + len(st.frame_bytes[1])), extra
    # a stream without a candidate: everything in front of L - 15 is decided (skipped), the rest held
    s = sm.Online(W)
    assert s.feed(bytes(100)) == [] and (s.base, len(s.tail), s.summary()) == (85, 15, (0, 85, 1))
    assert s.feed(bytes(5)) == [] and (s.base, len(s.tail), s.summary()) == (90, 15, (0, 90, 1))   # the same gap
    assert s.feed(b"", True) == [] and (s.base, len(s.tail), s.summary()) == (105, 0, (0, 105, 1))


def test_the_held_tail_never_exceeds_W_plus_15():
    blob, true_at = sm.lookalike_stream()
    w = W
    assert sm.raw_links_within(blob, w)
    worst = 0
    for step in (1, 7, 64, 333):
        cuts = list(range(step, len(blob), step)) + [len(blob)]
        feeds, summary, held = sm.online(blob, cuts, set(), w)
        want, want_summary = sm.segments(blob, (), w)
        assert sm.tuples([r for f in feeds for r in f]) == sm.tuples(want) and summary == want_summary
        assert want[0]["byte_offset"] == true_at and len(want) == len(rf.uniform().frame_bytes)
        assert held <= w + 15
        worst = max(worst, held)
    assert worst == w + 15   # reached, fed byte by byte: the look-alike with W + 15 bytes behind its first
    # fed byte by byte the look-alike is held until 16 bytes lie W behind it, then passed over
    s = sm.Online(w)
    for fed in range(1, w + 17):
        assert s.feed(blob[fed - 1:fed]) == []
        assert (s.base == 0) == (fed < w + 16), fed
    assert s.summary() == (0, s.base, 1)
