"""The cases and the float64 reference of tests/test_enroll.py and tests/test_enroll_gpu.py: speaker enrolment, i.e. the gradient of the
noise-prediction MSE with respect to `class_embed` and AdamW on it (reference train_vqvae_add.py, train_loop.py:438-485, 76).

The reference is `oracle.ref_cpu.unet_predictor` on a float64 state dict whose `class_embed.weight` is a float64 leaf: loss = the mean
over clips of the clip's MSE, `torch.autograd.grad` gives the table's gradient [num_labels, E]; the gradient of one clip's own MSE with
respect to its own vector is obtained the same way, one clip at a time, and so is the gradient with respect to every block's
`cond_layers.1.bias`, which for one clip IS (d a | d b) of that block: the float64 sums of du2 * h^ and of du2.  AdamW is written out
from its definition in numpy float64.

The models are the smallest that reach every form of the new kernels (csrc/enroll_kernels.hip) and of the reused backward schedule:

  pg32       default topology, base 32, cond_channels 32: B = 3, T = 1792 (7 conditioning rows; the second level is 896 rows = 3.5
             partial-sum tiles), labels (1, 3, 1): concatenating, avg-pool, nearest-x2 and 1x1-skip blocks; two clips on one row
  pg_ragged  channel_mult (1, 2, 2), depth_mult 1, middle_dilations (4,), no conditioning: B = 2, T = 592 (levels 592 / 296 / 148:
             whole and ragged tiles, single tiles); in down_blocks.1 the FiLM rows of channel 5 have weight 0 and bias -1 for `a`,
             so 1 + a = 0 exactly there: an implementation that derives d a from GroupNorm's sums divides by zero
  pg96       base 96, the same small topology, conditioning of an arbitrary length (5 rows: length code 1000 + 5), B = 2: octet
             counts that are no power of two
"""
import math
import os

import numpy as np
import torch

from oracle import ref_cpu
from vq_voice_swap_amd import UNetPredictor
from vq_voice_swap_amd.det_init import det_init_

SMALL = dict(channel_mult=(1, 2, 2), depth_mult=1, middle_dilations=(4,))
CASES = [
    dict(id="pg32", base=32, topo=None, cond_channels=32, cond_len=7, num_labels=5, B=3, T=1792, labels=(1, 3, 1), ts=(0.15, 0.5, 0.85),
         prefix="enr.pg32.", seed=8101),
    dict(id="pg_ragged", base=32, topo=SMALL, cond_channels=None, cond_len=0, num_labels=4, B=2, T=592, labels=(0, 2), ts=(0.3, 0.8),
         prefix="enr.pg_ragged.", seed=8102, zero_film=("down_blocks.1", 5)),
    dict(id="pg96", base=96, topo=SMALL, cond_channels=32, cond_len=5, num_labels=3, B=2, T=592, labels=(2, 0), ts=(0.25, 0.7),
         prefix="enr.pg96.", seed=8103),
]
CASE = {c["id"]: c for c in CASES}

MARGINS = "enroll_margins.jsonl"
GRAD_GATE_CAP = 2e-3  # the project's fp32 gradient figure (tests/backward_ref.py): no gate below may exceed it
# Gates of the GPU file, relative RMS against the float64 reference.  Each is `gate_of` of the recorded run
# profiles/enroll_margins.jsonl (tests/test_enroll.py checks that it is): 3 x the largest recorded value, rounded up to one
# significant digit, never above GRAD_GATE_CAP.  3 x: the kernels are deterministic on fixed inputs, so only the CU count (it
# regroups conv_ws_kernel's walks) and the compiler version can move a value.
#   grad   per-clip gradient d mse_b / d v_b, over the batch and for the worst clip, every case
#   dfilm  (d a | d b) of every block, over the batch and for the worst clip, every case
#   dfilm_block  (d a | d b) of every single block over the batch (the largest per case is recorded with the dfilm record)
#   adamw  the AdamW kernel: rows after 5 steps, error relative to the reference's displacement from the initial rows
#   traj   rows after 3 enrolment steps, error relative to the reference's displacement from the initial rows
GATES = {"grad": 2e-4, "dfilm": 2e-4, "dfilm_block": 5e-4, "adamw": 1e-5, "traj": 5e-4}
GATE_FIELDS = {"grad": ("grad_err", "grad_err_worst_clip"), "dfilm": ("dfilm_err", "dfilm_err_worst_clip"), "dfilm_block": ("worst_block_err",),
               "adamw": ("rows_err",), "traj": ("traj_err",)}
GATE_TEST = {"dfilm_block": "dfilm"}  # (the gate reads a field of another test's records)


def gate_of(records, test):
    """3 x the largest error that `records` hold for `test`, rounded up to one significant digit, never above GRAD_GATE_CAP."""
    errs = [r[f] for r in records if r.get("test") == "enroll." + GATE_TEST.get(test, test) for f in GATE_FIELDS[test]]
    v = 3.0 * max(errs)
    e = math.floor(math.log10(v))
    return min(GRAD_GATE_CAP, float(f"{math.ceil(v / 10.0 ** e - 1e-9)}e{e}"))


def recorded():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", MARGINS)
    import json

    return [json.loads(ln) for ln in open(path)]


def topology(case):
    return dict(case["topo"]) if case["topo"] else None


def make_model(case):
    """The predictor of a case on the CPU: det_init_ under the case's prefix, the FiLM patch of pg_ragged, eval()."""
    m = UNetPredictor(case["base"], cond_channels=case["cond_channels"], num_labels=case["num_labels"], **(case["topo"] or {}))
    det_init_((case["prefix"] + k, v) for k, v in m.state_dict().items())
    if "zero_film" in case:
        block, c = case["zero_film"]
        lin = dict(m.named_modules())[block].cond_layers[1]
        with torch.no_grad():
            lin.weight[c].zero_()  # row c of (a | b) is a_c
            lin.bias[c] = -1.0
    return m.eval()


def inputs(case):
    """(x_t [B, 1, T], ts [B], eps [B, 1, T], cond [B, Cc, L] or None, labels [B]) in float32 / int64, from the case's seed."""
    g = torch.Generator().manual_seed(case["seed"])
    B, T = case["B"], case["T"]
    x_t = torch.randn((B, 1, T), generator=g)
    eps = torch.randn((B, 1, T), generator=g)
    cond = torch.randn((B, case["cond_channels"], case["cond_len"]), generator=g) if case["cond_channels"] else None
    return x_t, torch.tensor(case["ts"], dtype=torch.float32), eps, cond, torch.tensor(case["labels"], dtype=torch.int64)


def film_rows(case):
    """[(block name, first row, cout)] of the [B, R] FiLM-gradient buffer: down, middle, up blocks, 2 * cout rows (d a | d b) each."""
    specs = ref_cpu.predictor_block_specs(case["base"], **(topology(case) or {}))
    out, row = [], 0
    for part, key in (("down_blocks", "down"), ("middle_blocks", "middle"), ("up_blocks", "up")):
        for i, spec in enumerate(specs[key]):
            out.append((f"{part}.{i}", row, spec["cout"]))
            row += 2 * spec["cout"]
    return out


def _f64_state(model, prefix="predictor."):
    return {prefix + k: v.detach().to(torch.float64) for k, v in model.state_dict().items()}


def clip_mses(sd, case, x_t, ts, eps, cond, labels):
    """[B] float64 MSE of every clip, differentiable, and the prediction."""
    pred = ref_cpu.unet_predictor(sd, case["base"], x_t, ts, cond=cond, labels=labels, topology=topology(case))
    return ((eps - pred) ** 2).flatten(1).mean(dim=1), pred


def reference(case, model=None, table=None, labels=None, data=None):
    """The float64 reference of a case: dict(pred [B, 1, T], mses [B], table_grad [num_labels, E] of the batch-mean loss, grads [B, E]
    of every clip's own MSE with respect to its own vector, dfilm [B, R]).  `table` / `labels` replace class_embed.weight and the
    case's labels (the enrolment trajectory runs on the new rows alone); `data` replaces `inputs(case)`."""
    m = model if model is not None else make_model(case)
    sd = _f64_state(m)
    x_t, ts, eps, cond, lab = data if data is not None else inputs(case)
    if labels is not None:
        lab = labels
    x_t, ts, eps = x_t.double(), ts.double(), eps.double()
    cond = None if cond is None else cond.double()
    W = (sd["predictor.class_embed.weight"] if table is None else table.double()).clone().requires_grad_(True)
    sd["predictor.class_embed.weight"] = W
    rows = film_rows(case)
    biases = []
    for name, _row, _cout in rows:
        key = f"predictor.{name}.cond_layers.1.bias"
        sd[key] = sd[key].clone().requires_grad_(True)
        biases.append(sd[key])
    mses, pred = clip_mses(sd, case, x_t, ts, eps, cond, lab)
    (table_grad,) = torch.autograd.grad(mses.mean(), W, retain_graph=False)
    B = x_t.shape[0]
    grads, dfilm = [], []
    for b in range(B):  # one clip at a time
        c1 = None if cond is None else cond[b:b + 1]
        mb, _ = clip_mses(sd, case, x_t[b:b + 1], ts[b:b + 1], eps[b:b + 1], c1, lab[b:b + 1])
        got = torch.autograd.grad(mb[0], [W] + biases)
        grads.append(got[0][lab[b]])
        dfilm.append(torch.cat(got[1:]))
    return dict(pred=pred.detach(), mses=mses.detach(), table_grad=table_grad.detach(), grads=torch.stack(grads).detach(),
                dfilm=torch.stack(dfilm).detach())


def adamw_ref(rows, m, v, grads, row_of_clip, step, lr, betas, eps, weight_decay):
    """One AdamW step from its definition (Loshchilov & Hutter, as torch.optim.AdamW evaluates it), numpy float64, returning the new
    (rows, m, v).  The gradient of a row is the sum over the clips that name it of the per-clip gradients, divided by the batch."""
    rows, m, v, grads = (np.asarray(a, dtype=np.float64) for a in (rows, m, v, grads))
    g = np.zeros_like(rows)
    for b, r in enumerate(np.asarray(row_of_clip).tolist()):
        g[r] += grads[b]
    g /= len(grads)
    b1, b2 = betas
    rows = rows * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    rows = rows - (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps)
    return rows, m, v


def f32(x):
    """A hyper-parameter as the C ABI receives it: rounded to float32, widened back."""
    return float(np.float32(x))


def trajectory_ref(case, rows0, new_labels, steps, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, model=None, data=None):
    """Reference autograd plus reference AdamW on a fixed batch (`data`, else the inputs of `case`): ([rows after step k], [batch-mean
    loss before step k])."""
    m = model if model is not None else make_model(case)
    rows = rows0.double().numpy().copy()
    mom, var = np.zeros_like(rows), np.zeros_like(rows)
    out, losses = [], []
    for k in range(1, steps + 1):
        r = reference(case, m, table=torch.from_numpy(rows), labels=new_labels, data=data)
        losses.append(r["mses"].mean().item())
        rows, mom, var = adamw_ref(rows, mom, var, r["grads"].numpy(), new_labels.tolist(), k, f32(lr), (f32(betas[0]), f32(betas[1])),
                                   f32(eps), f32(weight_decay))
        out.append(rows.copy())
    return out, losses


def rel_rms(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return ((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()


def clip_rel_rms(got, want):
    got, want = torch.as_tensor(got).double().flatten(1), torch.as_tensor(want).double().flatten(1)
    return (got - want).pow(2).mean(dim=1).sqrt() / want.pow(2).mean(dim=1).sqrt()
