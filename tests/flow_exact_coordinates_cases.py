"""The fused flow pass at the shapes where its pixel coordinates can go wrong: what tools/make_golden_flow_exact_coordinates.py records from
one commit and tests/test_gpu_flow_exact_coordinates.py compares a later one against, bit for bit.  Inputs, entry points and outputs are
those of tests/flow_frame_constants_cases.py (seeded inputs, ``Problem``); only the shapes are others.

The kernel walks (row, quad in the row) with integer adds — 256 items further per iteration — and takes the pixel centres (i + 0.5) / n from
a host reciprocal with one correction step (pixel_center_recip, fm_math.h) where both dimensions are at most 16 384.  Neither may show in an
output.  Three frames each: the first lacks the backward term, the last the forward one, the interior one has both.
"""

import flow_frame_constants_cases as fc

# (B, F, H, W).  One workgroup per frame (at most 1 024 items): every sum receives one fp64 atomic onto zero, every output reproduces itself.
ONE_WORKGROUP_SHAPES = [(1, 3, 1024, 4),  # one quad per row: the row advances 256 per iteration, the column never
                        (1, 3, 500, 8),   # two quads per row
                        (1, 3, 4, 1020),  # 255 quads per row, one short of the workgroup: the column steps back by one, with a carry
                        (1, 3, 4, 1024),  # 256 quads per row: a thread stays in its column, the row advances by one
                        (1, 3, 3, 1028),  # 257 quads per row: the walk's whole-row step is 0
                        (1, 3, 100, 5),   # W % 4 != 0: one pixel per item
                        (1, 3, 700, 1)]   # ... and one pixel per row
TWO_WORKGROUP_SHAPE = (1, 3, 8, 1020)     # 2 040 quads per frame: the second workgroup starts inside a row
BEYOND_PROVEN_RANGE_SHAPE = (1, 3, 1, 16388)  # W > 16 384: the dividing path (five workgroups per frame)
ATOMIC_SHAPES = [TWO_WORKGROUP_SHAPE, BEYOND_PROVEN_RANGE_SHAPE]  # sums meet through fp64 atomics: 1e-6 relative (include/flowmap_hip.h)
SHAPES = ONE_WORKGROUP_SHAPES + ATOMIC_SHAPES


def combos(shapes=None):
    """(shape, kind, format, gradients?) of every recorded case."""
    for shape in SHAPES if shapes is None else shapes:
        for kind in fc.KINDS:
            for fmt in fc.formats_of(shape):
                for grad in (True, False):
                    yield shape, kind, fmt, grad
