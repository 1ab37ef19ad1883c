import torch


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_rms(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-12)).item()


def rms(a):
    return a.pow(2).mean().sqrt().item()


def flags_of(parser):
    return sorted(s for a in parser._actions for s in (a.option_strings or [a.dest]) if s not in ("-h", "--help"))


def run_script(script, args, ranks=1, seconds=300):
    """A script of the repository root as one fresh child process under its own time limit (`ranks` > 1: that many gloo ranks under
    torch.distributed.run); a failing child fails the test at once.  Returns the whole stdout."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    launch, tail = [sys.executable], []
    if ranks > 1:
        from bench import free_port

        env["OMP_NUM_THREADS"] = "2"
        launch += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port())]
        tail = ["--dist-backend", "gloo"]
    cmd = ["timeout", "-k", "10", str(seconds)] + launch + [os.path.join(root, script)] + [str(a) for a in args] + tail
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def sample_lines(stdout):
    """The "{n} samples: ..." lines of an eval script's output."""
    return [ln for ln in stdout.splitlines() if " samples: " in ln]


def record_margin(file_name, rec):
    """Print one measured margin and, when the environment names a directory in VQVS_MARGINS_DIR, append it to <file_name>
    there (the print-and-append half of `gate`, for gates that are not an RMS of a waveform; a GPU run's records are kept under
    profiles/)."""
    import json
    import os

    print("[margin] " + json.dumps(rec))
    out = os.environ.get("VQVS_MARGINS_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, file_name), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def gate(name, got, want, bound, relative=False):
    """Waveform gate: assert RMS(got - want) < bound (relative to RMS(want) when `relative`; bound None = record the value without
    gating it, only a gross-error check at 1e-2 stays), print the measured value and
    append it to gpurun_out/parity_margins.jsonl (the margins are recorded under profiles/ from a GPU run).  For bounded
    (constrained) waveforms the RMS over the samples the reference did NOT clamp to +-1 is recorded too: clamped samples hide
    error."""
    import json
    import os

    d = got - want
    val = rel_rms(got, want) if relative else rms(d)
    rec = {"test": name, "rms": val, "bound": bound, "relative": bool(relative)}
    if not relative:
        unsat = want.abs() < 1.0
        rec["saturated_fraction"] = 1.0 - unsat.float().mean().item()
        rec["rms_unsaturated"] = d[unsat].pow(2).mean().sqrt().item() if unsat.any() else 0.0
    rec["gated"] = bound is not None
    if bound is None:
        bound = rec["bound"] = 1e-2
    print(f"[margin] {name}: {'rel ' if relative else ''}rms {val:.3e} ({'bound' if rec['gated'] else 'NOT GATED, gross-error bound'} {bound:.1e})"
          + ("" if relative else f", unsaturated-only {rec['rms_unsaturated']:.3e}, saturated {rec['saturated_fraction']:.2f}"))
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "parity_margins.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert val < bound, (name, val, bound)
    return val
