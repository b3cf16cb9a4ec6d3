"""Many seeds and degenerate-but-legal inputs through the full step and the sampled fit (tests/adversarial_cases.py) against the
fp64 oracle — on the GPU: the same lists as the CPU module, plus the full-size frame on two seeds."""

import pytest

import adversarial_cases as adv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("cfg", adv.sweep_configs() + adv.sweep_configs(adv.SWEEP_FULL_SIZE, seeds=(0, 1), first=2), ids=adv.sweep_id)
def test_seed_sweep_gpu(cfg):
    adv.case_seed_sweep(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.fit_configs(), ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}-s{c[4]}")
def test_fit_per_pair_gpu(cfg):
    adv.case_fit_per_pair(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.regime_configs(), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-P{c[4]}-{c[5]}")
def test_regime_gpu(cfg):
    adv.case_regime(DEV, cfg)


@pytest.mark.parametrize("cfg", adv.TINY_FRAMES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}")
def test_tiny_frame_gpu(cfg):
    adv.case_tiny_frame(DEV, cfg)


@pytest.mark.parametrize("scale", adv.DEPTH_SCALES)
def test_scaled_scene_gpu(scale):
    adv.case_scaled_scene(DEV, scale)


def test_two_frames_with_tracks_gpu():
    adv.case_two_frames_with_tracks(DEV)


def test_nothing_visible_gpu():
    adv.case_nothing_visible(DEV)


def test_one_frame_segments_gpu():
    adv.case_one_frame_segments(DEV)


@pytest.mark.parametrize("points", (3, 4))
def test_few_points_gpu(points):
    adv.case_few_points(DEV, points)


@pytest.mark.parametrize("points", (1, 2))
def test_too_few_points_gpu(points):
    adv.case_too_few_points(DEV, points)
