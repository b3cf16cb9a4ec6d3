"""What the residual bench tools (bench_flow_residuals, bench_track_residuals, bench_alignment_residuals, bench_focal_sweep) share: the
device-event timer, the HBM peak their shares refer to, the alternating rounds of fresh child processes and the summary over the rounds."""

from __future__ import annotations

import json
import statistics
import subprocess
import sys
from pathlib import Path

HBM_PEAK = 8.0e12  # bytes/s (MI355X)


def timed(fn, iters, warmup=2):
    """ms per call of ``fn``: device events around ``iters`` calls after ``warmup`` calls."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def child_rounds(tool, script, common, routes, rounds, step_timeout):
    """{route: [the child's result per round]}: ``rounds`` times over ``routes``, ``script`` with ``common + ["--child", route]`` in a fresh
    process under its own limit, its result the JSON after "RESULT " on its last such line.  A failure or a timeout ends the run: nothing
    more is started on the GPU."""
    runs = {route: [] for route in routes}
    for _ in range(rounds):
        for route in routes:
            done = subprocess.run([sys.executable, str(Path(script).resolve()), *common, "--child", route], capture_output=True, text=True, timeout=step_timeout)
            lines = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")]
            if done.returncode != 0 or not lines:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-2000:])
                raise SystemExit(f"{tool}: the {route} measurement failed (exit status {done.returncode}); stopping")
            runs[route].append(json.loads(lines[-1][len("RESULT "):]))
    return runs


def print_child_result(result):
    print("RESULT " + json.dumps(result), flush=True)


def summary(results, name, scale_to_median=()):
    """Measurement ``name`` over one route's rounds: the first round's fields with ``ms`` = the median and ``ms_min`` / ``ms_max`` added;
    the rates named in ``scale_to_median`` are taken at the median time.  Floats rounded to four places."""
    ms = [r[name]["ms"] for r in results]
    median = statistics.median(ms)
    out = dict(results[0][name], ms=median, ms_min=min(ms), ms_max=max(ms))
    for key in scale_to_median:
        if key in out:
            out[key] = out[key] * ms[0] / median
    return {key: (round(v, 4) if isinstance(v, float) else v) for key, v in out.items()}


def emit(result, out=None):
    """The tool's one JSON line, printed and — with ``out`` — written to that file."""
    line = json.dumps(result)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")
