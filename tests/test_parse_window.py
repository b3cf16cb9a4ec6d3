"""flowmap_amd._base.parse_window: the one parser of the ``pairs`` / ``segments`` argument of the residual calls (LossFlow.residuals,
LossTracking.residuals, alignment_residuals, focal_sweep) — every accepted form, every refused one, and the caller's name in the text."""

import re

import pytest

from flowmap_amd._base import parse_window

TOTAL = 5
# (selection, allow_int, (first, count)) — or an error pattern after "flowmap_amd: {what}" in place of the pair
TABLE = [
    (None, False, (0, 5)),
    (None, True, (0, 5)),
    (slice(None), False, (0, 5)),
    (slice(1, 3), False, (1, 2)),
    (slice(1, 3, 1), False, (1, 2)),
    (slice(-2, None), False, (3, 2)),  # a negative start counts from the end
    (slice(-4, -1), False, (1, 3)),
    (slice(0, 99), False, (0, 5)),  # a slice is clipped as a sequence clips it
    (slice(0, 4, 2), False, r" takes a slice of {noun} with step 1 \(got step 2\)"),
    (slice(None, None, -1), False, r" takes a slice of {noun} with step 1 \(got step -1\)"),
    (slice(3, 1), False, r": the {noun} \[3, 1\) do not lie in the 5 {noun}"),  # empty
    (slice(5, None), False, r": the {noun} \[5, 5\) do not lie in the 5 {noun}"),
    ((1, 2), False, (1, 2)),
    ((0, 5), False, (0, 5)),
    ((4, 1), False, (4, 1)),
    ([3, 1], False, (3, 1)),
    ((0, 0), False, r": the {noun} \[0, 0\) do not lie in the 5 {noun}"),
    ((3, 3), False, r": the {noun} \[3, 6\) do not lie in the 5 {noun}"),
    ((-1, 2), False, r": the {noun} \[-1, 1\) do not lie in the 5 {noun}"),  # (first, count) does not wrap
    ((0, 6), False, r": the {noun} \[0, 6\) do not lie in the 5 {noun}"),
    ((0, 1, 2), False, r": {noun} must be None, a slice with step 1 or \(first, count\), got \(0, 1, 2\)"),
    ((1.0, 2), False, r": {noun} must be None, a slice with step 1 or \(first, count\), got \(1\.0, 2\)"),
    ((True, 2), False, r": {noun} must be None, a slice with step 1 or \(first, count\), got \(True, 2\)"),  # bools are no ints here
    ((1, False), True, r": {noun} must be None, an int, a slice with step 1 or \(first, count\), got \(1, False\)"),
    ("all", False, r": {noun} must be None, a slice with step 1 or \(first, count\), got 'all'"),
    (2, False, r": {noun} must be None, a slice with step 1 or \(first, count\), got 2"),  # an int only with allow_int
    (2, True, (2, 1)),
    (0, True, (0, 1)),
    (-1, True, (4, 1)),  # a negative int wraps
    (-5, True, (0, 1)),
    (5, True, r": the {noun} \[5, 6\) do not lie in the 5 {noun}"),
    (-6, True, r": the {noun} \[-1, 0\) do not lie in the 5 {noun}"),
    (True, True, r": {noun} must be None, an int, a slice with step 1 or \(first, count\), got True"),
    (1.0, True, r": {noun} must be None, an int, a slice with step 1 or \(first, count\), got 1\.0"),
]


@pytest.mark.parametrize("what,noun", [("LossFlow.residuals", "pairs"), ("focal_sweep", "pairs"), ("LossTracking.residuals", "segments")])
def test_every_form(what, noun):
    for selection, allow_int, want in TABLE:
        if isinstance(want, tuple):
            got = parse_window(selection, TOTAL, what, noun, allow_int=allow_int)
            assert got == want and all(type(v) is int for v in got), f"{selection!r}: {got}"
        else:
            with pytest.raises(ValueError, match="^" + re.escape(f"flowmap_amd: {what}") + want.format(noun=noun)):
                parse_window(selection, TOTAL, what, noun, allow_int=allow_int)


def test_the_callers_name_their_own_call():
    """The window of the whole video is one pair wide here: every public caller refuses pair 1 under its own name."""
    with pytest.raises(ValueError, match=r"^flowmap_amd: alignment_residuals: the pairs \[1, 2\) do not lie in the 1 pairs of the video$"):
        parse_window((1, 1), 1, "alignment_residuals", "pairs")
    with pytest.raises(ValueError, match=r"^flowmap_amd: LossTracking\.residuals: the segments \[1, 2\) do not lie in the 1 segments of the track list$"):
        parse_window(1, 1, "LossTracking.residuals", "segments", allow_int=True)
