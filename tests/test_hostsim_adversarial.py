"""Many seeds and degenerate-but-legal inputs through the full step and the sampled fit (tests/adversarial_cases.py) against the
fp64 oracle — CPU, host double."""

import pytest

import adversarial_cases as adv
from flowmap_amd import _lib
from helpers import build_host_sim

DEV = "cpu"


@pytest.fixture(autouse=True, scope="module")
def host_double():
    _lib.set_library_for_testing(build_host_sim())
    yield
    _lib.set_library_for_testing(None)


@pytest.mark.parametrize("cfg", adv.sweep_configs(), ids=adv.sweep_id)
def test_seed_sweep(cfg):
    adv.case_seed_sweep(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.fit_configs(), ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}-s{c[4]}")
def test_fit_per_pair(cfg):
    adv.case_fit_per_pair(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.regime_configs(), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-P{c[4]}-{c[5]}")
def test_regime(cfg):
    adv.case_regime(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.TINY_FRAMES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}")
def test_tiny_frame(cfg):
    adv.case_tiny_frame(DEV, cfg)


@pytest.mark.parametrize("scale", adv.DEPTH_SCALES)
def test_scaled_scene(scale):
    adv.case_scaled_scene(DEV, scale)


def test_two_frames_with_tracks():
    adv.case_two_frames_with_tracks(DEV)


def test_nothing_visible():
    adv.case_nothing_visible(DEV)


def test_one_frame_segments():
    adv.case_one_frame_segments(DEV)


@pytest.mark.parametrize("points", (3, 4))
def test_few_points(points):
    adv.case_few_points(DEV, points)


@pytest.mark.parametrize("points", (1, 2))
def test_too_few_points(points):
    adv.case_too_few_points(DEV, points)
