"""The shared evaluation pass (vq_voice_swap_amd/eval_pass.py) on the host: the loop deals the batches and the merge collects them
alike at 1, 2 and 3 ranks (gloo, a fake state on device "cpu"); the common parser; the one `format_line`."""
import json
import os
import subprocess
import sys

import pytest

from vq_voice_swap_amd import eval_pass

from util import flags_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, os, sys
from fractions import Fraction
sys.path.insert(0, {root!r})
from vq_voice_swap_amd import create_data_loader
from vq_voice_swap_amd.eval_pass import close_ranks, merge_ranks, open_ranks, score_batches

class Fake:   # the state protocol, recording what the loop hands over
    def __init__(self):
        self.batches, self.num_samples, self.total, self.on_host = [], 0, Fraction(0), False
    def add(self, audio, data_batch, first):
        assert audio.dim() == 3 and audio.shape[1] == 1 and audio.device.type == "cpu"
        self.batches.append((first, data_batch["label"].tolist()))
        self.num_samples += len(audio)
        self.total += Fraction(float(data_batch["samples"].double().sum()))
    def merge(self, other):
        assert other.on_host
        self.batches += other.batches
        self.num_samples += other.num_samples
        self.total += other.total
        return self
    def to_host(self):
        self.on_host = True
        return self
    def log_dict(self):
        return {{"batches": len(self.batches)}}

rank, world = open_ranks("gloo")
import torch.distributed as dist
assert world == int(os.environ["WORLD_SIZE"]) and dist.is_initialized() == (world > 1)  # one rank opens no process group
loader, num_labels = create_data_loader("tones", batch_size=2, seed=1, rank=rank, world=world)
state = Fake()
score_batches(loader, state, state.add, "cpu", batch_size=2, max_samples=7, rank=rank, world=world)
assert [first % (2 * world) for first, _ in state.batches] == [2 * rank] * len(state.batches)  # this rank's batches, and only they
merged = merge_ranks(state, rank, world)
if rank == 0:
    assert merged is state
    print("RESULT " + json.dumps({{"batches": sorted(merged.batches), "num_samples": merged.num_samples,
                                   "total": [merged.total.numerator, merged.total.denominator]}}))
else:
    assert merged is None
close_ranks(world)
"""


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    """stdout of the worker at 1, 2 and 3 ranks."""
    from bench import free_port

    script = tmp_path_factory.mktemp("eval_pass") / "w.py"
    script.write_text(WORKER.format(root=ROOT))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    runs = {ranks: subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
                                     "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script)],
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for ranks in (1, 2, 3)}  # six processes at once
    out = {}
    for ranks, run in runs.items():
        stdout, stderr = run.communicate()
        assert run.returncode == 0, stdout[-2000:] + stderr[-4000:]
        out[ranks] = stdout.splitlines()
    return out


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_loop_deals_and_merges_alike_at_every_rank_count(passes, ranks):
    results = {n: [json.loads(ln[len("RESULT "):]) for ln in lines if ln.startswith("RESULT ")] for n, lines in passes.items()}
    assert len(results[ranks]) == 1  # rank 0 alone holds a merged state
    got = results[ranks][0]
    # the pass of seed 1 in batches of 2; the batch at 6 is refused: 6 + 2 > 7
    assert got["batches"] == [[0, [1, 1]], [2, [0, 2]], [4, [2, 0]]] and got["num_samples"] == 6
    assert got["total"] == results[1][0]["total"]  # the exact sum over the six clips
    lines = [ln for ln in passes[ranks] if " samples: " in ln]
    if ranks == 1:
        assert lines == ["2 samples: batches=1", "4 samples: batches=2", "6 samples: batches=3"]
    else:
        assert lines == ["6 samples: batches=3"]


def test_common_parser_parses_as_the_scripts_did():
    import eval_classifier
    import eval_conversion
    import eval_diffusion
    import eval_enc_pred
    import eval_vqvae

    a = eval_pass.common_parser().parse_args(["model.pt", "tones"])
    assert (a.batch_size, a.precision, a.seed, a.max_samples, a.dist_backend) == (4, "fp32", 0, None, "nccl")
    assert (a.checkpoint_path, a.data_dir) == ("model.pt", "tones")
    a = eval_pass.common_parser().parse_args(["--batch-size", "3", "--precision", "bf16", "--seed", "5", "--max-samples", "9", "--dist-backend", "gloo",
                                              "model.pt", "data/"])
    assert (a.batch_size, a.precision, a.seed, a.max_samples, a.dist_backend) == (3, "bf16", 5, 9, "gloo")
    for bad in (["--precision", "fp8"], ["--dist-backend", "mpi"]):
        with pytest.raises(SystemExit):
            eval_pass.common_parser().parse_args(bad + ["model.pt", "tones"])
    common = ["--batch-size", "--precision", "--seed", "--max-samples", "--dist-backend", "checkpoint_path", "data_dir"]
    assert flags_of(eval_pass.common_parser()) == sorted(common)
    own = {eval_diffusion: [], eval_vqvae: [], eval_classifier: ["--schedule", "--t", "--topk", "--confusion-path"],
           eval_enc_pred: ["--topk", "--vq-vae-path"],
           eval_conversion: ["--sampler", "--eta", "--sample-steps", "--target", "--reference-steps", "--reference-sampler", "--classifier"]}
    for script, flags in own.items():
        assert flags_of(script.arg_parser()) == sorted(common + flags), script.__name__


def test_format_line_is_one_object():
    import eval_classifier
    import eval_conversion
    import eval_enc_pred
    import eval_vqvae

    assert eval_classifier.format_line is eval_vqvae.format_line is eval_conversion.format_line is eval_enc_pred.format_line is eval_pass.format_line
    assert eval_pass.format_line(3, {"used_codes": 7, "vq_loss": 0.5}) == "3 samples: used_codes=7 vq_loss=0.500000"
