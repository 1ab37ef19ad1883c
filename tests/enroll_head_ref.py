"""The cases, the reference and the error bound of tests/test_enroll_classifier.py and tests/test_enroll_classifier_gpu.py: classifier
enrolment, i.e. `vqvs_head_xent_grad` and `vqvs_head_adamw` (csrc/enroll_kernels.hip), `ClassifierEnroller` and enroll_classifier.py.

The reference.  Both calls take `act` = gelu_f(feat) as GIVEN (float32, what the kernel wrote): the head GELU is the library's own
f32 function and is held to its own tolerance separately.  `head_ref` restates the first call -- logits, nll, first-index argmax,
new_mass, coef -- and `grad_ref` / `adamw_update` the second, in numpy.  They run in float64, or, for the bound test, in numpy's
extended precision (x87 long double, unit roundoff 2^-64): a float64 reference has rounding errors of the same size as the float64
kernel it judges, an extended one has them 2^11 times smaller.  `AutogradHead` is the same step through float64 `torch.autograd` and
`torch.optim.AdamW` on a grown `nn.Linear`.

The bound of `vqvs_head_xent_grad` (u = 2^-53; everything per clip; N = K + n).
  logits.  logit_k = b_k + sum_f w_kf act_f.  A product of two float32 values has at most 48 significant bits: exact in float64.  So
    only the additions round.  The kernel adds the F products and the bias in a fixed tree: lane l of a wave chains f = l, l + 64, ...
    (at most ceil(F / 64) terms, the first addition, to 0, exact), six xor-shuffle levels fold the lanes (adding a lane that holds 0 is
    exact), the bias is added last.  A term therefore passes through at most D = min(F, ceil(F / 64) + 6) roundings: the tree's depth,
    and never more than F, the number of additions that are not additions of zero in ANY order of F + 1 terms.  Each rounding
    multiplies by (1 + e), |e| <= u, so
        |dlogit_k| <= ((1 + u)^D - 1) S_k <= (D + 1) u S_k =: E_k,      S_k = |b_k| + sum_f |w_kf act_f|
    (the extra unit absorbs the second-order terms: D u < 2^-40).  delta = max_k E_k.
  from here on the kernel's float64 logits l^ are the inputs, and an exact evaluation on l^ differs from the exact one on l by
    |lse(l^) - lse(l)| <= delta, |l^_y - l_y| <= delta            -> 2 delta on nll       (logsumexp is 1-Lipschitz in the max norm)
    |softmax(l^)_k - softmax(l)_k| <= p_k (e^(2 delta) - 1)       -> 2 delta on coef and on new_mass (a sum of p_k <= 1)
  the kernel's own roundings on l^, with d_k = l^_k - M <= 0, t_k = e^(d_k), S = sum t_k >= 1 (the maximum's term is exactly 1):
    d_k rounds once: |dd_k| <= u |d_k|.  exp and log of the device library are accurate to 1 ulp, a relative 2 u.  So
        |dt_k| <= t_k (u |d_k| + 2 u) <= u / e + 2 u t_k          (x e^-x <= 1 / e)
    S adds N non-negative terms; in any order the sum's own roundings are at most (N - 1) u S.  Together
        |dS| / S <= u (N / e + 2 S + (N - 1) S) / S <= u (2 N + 1)                                    (S >= 1)
    log S: |d log S| <= u (2 N + 1) + 2 u |log S| <= u (2 N + 1 + 2 ln N)                             (1 <= S <= N)
    nll = log S - d_y: d_y carries u |d_y|, the subtraction rounds once: u |nll|.
        E_nll  = 2 delta + u (2 N + 2 + 2 ln N + |d_y| + |nll|)
    p_j = t_j / S: relative u |d_j| + 2 u from t_j, u (2 N + 1) from S, u from the division; p_j |d_j| <= 1 / e, p_j <= 1; the
    subtraction of the indicator rounds once, |coef| <= 1.
        E_coef = 2 delta + u (2 N + 6)
    new_mass = S_new / S: S_new adds n of the same terms: |dS_new| <= u (n / e + 2 S_new + (n - 1) S_new), S_new <= S, S >= 1, so
    |dS_new| / S <= u (2 n + 1); the denominator adds u (2 N + 1) new_mass, the division u.
        E_mass = 2 delta + u (2 N + 2 n + 4)
  (each constant has one unit to spare for the second-order terms.)
The bound is derived, not measured: no test may widen it.  If the kernel breaks it, the derivation or the kernel is wrong; find which.
`share_of_bound` gives the largest fraction of it that an answer uses; the GPU file records it.

`vqvs_head_adamw` evaluates g and the update in float64 from float32 state and rounds once per stored value, so every stored value
is within 1 float32 ulp of the float64 result rounded to float32 (the float64 evaluations may differ in their last bits, which can
move a value across one rounding boundary, never two).
"""
import math
import os

import numpy as np
import torch

U = 2.0 ** -53
XL = np.longdouble  # extended precision of the bound test (unit roundoff 2^-64 on x86)

# (B, K, n, F) of the first call: one of everything; odd sizes; K + n = 256, the last width one thread-stride of the softmax loops
# covers, and 257, the first it does not; the workload's (8, 251, 4, 512); the K + n limit of 8192 (the LDS limit of the logits).
XENT_SHAPES = [(1, 1, 1, 1), (3, 5, 2, 33), (2, 250, 6, 63), (2, 251, 5, 64), (2, 252, 5, 65), (8, 251, 4, 512), (1, 8000, 192, 96)]
KINDS = ("plain", "saturated")  # "saturated": the head scaled so that the largest |logit| is 80 and the softmax saturates
ADAMW_B = (1, 3, 8)
ADAMW_WD = (0.0, 0.01)
ADAMW_STEPS = (1, 7)  # the steps whose stored values are compared (seven steps are run)
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)

MARGINS = "enroll_classifier_margins.jsonl"
# the feature vector's GELU against float64 erf-GELU: the absolute tolerance at which the project's parity tests hold the one value
# they compare that gelu_f forms directly, the conditioning vector of tests/test_parity_gpu.py::test_time_embedding_vs_golden
ACT_TOL = 2e-5
# Gate of the three-step test of the GPU file: `enroll_ref.gate_of` of the recorded run profiles/enroll_classifier_margins.jsonl
# (tests/test_enroll_classifier.py checks that it is): 3 x the largest recorded fp32 value, rounded up to one significant digit,
# never above enroll_ref.GRAD_GATE_CAP.  3 x: both head kernels are deterministic on fixed inputs, so only the stem's fp32 error
# (the CU count regroups conv_ws_kernel's walks; the compiler version) moves a value.
GATES = {"traj": 3e-5}
TRAJ_CASES = ("clf_f15a", "clf_ragged")  # the two smallest classifiers of tests/backward_ref.py


def recorded():
    import json

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", MARGINS)
    return [json.loads(ln) for ln in open(path)]


def f32(x):
    """A hyper-parameter as the C ABI receives it: rounded to float32, widened back."""
    return float(np.float32(x))


def gelu64(x):
    """erf-GELU in float64 (nn.GELU's default)."""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


# ---------------------------------------------------------------------------------------------------------------- the first call
def head_ref(act, w_old, b_old, rows, targets, dtype=np.float64):
    """The first call restated in `dtype` from `act` [B, F], `w_old` [K, F], `b_old` [K], `rows` [n, F + 1] (the kernel's are float32;
    a float64 trajectory's rows are taken as they are) and int `targets` [B]: dict(logits [B, N], mag [B, N] (S_k of the bound), nll, top1, new_mass [B], coef [B, n], d_y [B]).  Every row's
    logit is formed by the same expression, so bitwise-equal rows give bitwise-equal logits and ties are exact."""
    act, w_old, b_old, rows = (np.asarray(a).astype(dtype) for a in (act, w_old, b_old, rows))
    y = np.asarray(targets, dtype=np.int64)
    K = w_old.shape[0]
    W = np.concatenate([w_old, rows[:, :-1]], axis=0)
    b = np.concatenate([b_old, rows[:, -1]])
    prod = act[:, None, :] * W[None, :, :]  # [B, N, F]
    logits = prod.sum(axis=-1) + b[None, :]
    mag = np.abs(prod).sum(axis=-1) + np.abs(b)[None, :]
    M = logits.max(axis=1, keepdims=True)
    d = logits - M
    t = np.exp(d)
    S = t.sum(axis=1)
    rng = np.arange(len(y))
    d_y = d[rng, y]
    onehot = np.zeros_like(logits)
    onehot[rng, y] = 1
    p = t / S[:, None]
    return dict(logits=logits, mag=mag, nll=np.log(S) - d_y, top1=(logits.argmax(axis=1) == y).astype(np.int64),
                new_mass=t[:, K:].sum(axis=1) / S, coef=p[:, K:] - onehot[:, K:], d_y=d_y)


def bounds(ref, F, K, n):
    """(E_logit [B, N], E_nll [B], E_coef [B], E_mass [B]) of a `head_ref` result: the derivation is in the module docstring."""
    N = K + n
    D = min(F, -(-F // 64) + 6)
    E_logit = (D + 1) * U * ref["mag"].astype(np.float64)
    delta = E_logit.max(axis=1)
    E_nll = 2 * delta + U * (2 * N + 2 + 2 * math.log(N) + np.abs(ref["d_y"]).astype(np.float64) + np.abs(ref["nll"]).astype(np.float64))
    return E_logit, E_nll, 2 * delta + U * (2 * N + 6), 2 * delta + U * (2 * N + 2 * n + 4)


def share_of_bound(got, ref, F, K, n):
    """{"nll", "coef", "new_mass"}: the largest |got - ref| / bound over the clips (coef: over its entries); `ref` in extended precision."""
    _, E_nll, E_coef, E_mass = bounds(ref, F, K, n)

    def err(name):
        return np.abs(np.asarray(got[name], dtype=np.float64).astype(XL) - ref[name]).astype(np.float64)

    return {"nll": float((err("nll") / E_nll).max()), "coef": float((err("coef") / E_coef[:, None]).max()),
            "new_mass": float((err("new_mass") / E_mass).max())}


def make_case(shape, kind, seed=None):
    """Inputs of a shape: dict(feat [B, F], w_old, b_old, rows, targets) as float32 / int64 CPU tensors, never modified.
      * features N(0, 1.5^2) (|feat| up to ~6: both tails of the GELU), head and rows N(0, 1 / F), biases N(0, 0.01);
      * "saturated": head, rows and biases scaled by one factor so that the largest |logit| of the batch is 80;
      * duplicated rows: the row that holds clip 0's maximum is copied over the last row (over row 0 if it IS the last), so the two
        tie bitwise; clip 0's target is the first of the pair (top1 = 1), clip 1 repeats clip 0 with the second as its target (top1 = 0);
      * the other clips take new labels (even b) and old ones (odd b) in turn."""
    B, K, n, F = shape
    g = torch.Generator().manual_seed(9300 + 7 * XENT_SHAPES.index(shape) + KINDS.index(kind) if seed is None else seed)
    feat = 1.5 * torch.randn(B, F, generator=g)
    if B > 1:
        feat[1] = feat[0]
    full = torch.cat([torch.randn(K + n, F, generator=g) / math.sqrt(F), 0.1 * torch.randn(K + n, 1, generator=g)], dim=1)
    act = torch.from_numpy(gelu64(feat.numpy())).float()

    def logits_of(rows_full):
        return head_ref(act.numpy(), rows_full[:K, :-1].numpy(), rows_full[:K, -1].numpy(), rows_full[K:].numpy(), np.zeros(B, dtype=np.int64))["logits"]

    if kind == "saturated":
        full = (full * (80.0 / float(np.abs(logits_of(full)).max()))).float()
    a = int(logits_of(full)[0].argmax())
    lo, hi = (a, K + n - 1) if a != K + n - 1 else (0, a)
    full[hi if a == lo else lo] = full[a]
    targets = torch.tensor([K + (b % n) if b % 2 == 0 else b % K for b in range(B)], dtype=torch.int64)
    targets[0] = lo
    if B > 1:
        targets[1] = hi
    return dict(feat=feat.contiguous(), w_old=full[:K, :-1].contiguous(), b_old=full[:K, -1].contiguous(), rows=full[K:].contiguous(),
                targets=targets, tie=(lo, hi))


# ---------------------------------------------------------------------------------------------------------------- the second call
def grad_ref(act, coef):
    """g [n, F + 1] = (sum_b coef[b, j] * act[b, f]) / B with act[b, F] = 1, float64: nlls.mean().backward() on the new rows."""
    act, coef = np.asarray(act, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    ext = np.concatenate([act, np.ones((act.shape[0], 1))], axis=1)
    return np.einsum("bj,bf->jf", coef, ext) / act.shape[0]


def adamw_update(rows, m, v, g, step, lr, betas, eps, weight_decay):
    """One AdamW step from its definition (Loshchilov & Hutter, as torch.optim.AdamW evaluates it), numpy float64: (rows, m, v)."""
    rows, m, v, g = (np.asarray(a, dtype=np.float64) for a in (rows, m, v, g))
    b1, b2 = betas
    rows = rows * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    rows = rows - (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps)
    return rows, m, v


def step_ref(act, w_old, b_old, rows, m, v, targets, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """Both calls in float64: (rows, m, v) after the step, and the `head_ref` result before it."""
    r = head_ref(act, w_old, b_old, rows, targets)
    return adamw_update(rows, m, v, grad_ref(act, r["coef"]), step, lr, betas, eps, weight_decay) + (r,)


def trajectory_ref(act, w_old, b_old, rows0, targets, steps, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """`steps` float64 steps on one fixed batch: ([rows after step k], [batch-mean NLL before step k])."""
    rows = np.asarray(rows0, dtype=np.float64).copy()
    m, v = np.zeros_like(rows), np.zeros_like(rows)
    out, losses = [], []
    for k in range(1, steps + 1):
        rows, m, v, r = step_ref(act, w_old, b_old, rows, m, v, targets, k, f32(lr), (f32(betas[0]), f32(betas[1])), f32(eps), f32(weight_decay))
        losses.append(float(r["nll"].mean()))
        out.append(rows.copy())
    return out, losses


class AutogradHead:
    """The same steps through float64 `torch.autograd` and `torch.optim.AdamW` on a grown `nn.Linear(F, K + n)`.  The optimiser owns
    the whole weight and bias; the old rows are frozen by writing the checkpoint's values back after every step (AdamW is
    element-wise, so what it did to them never reaches the new rows)."""

    def __init__(self, w_old, b_old, rows0, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        w_old, b_old, rows0 = (torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (w_old, b_old, rows0))
        self.K = w_old.shape[0]
        self.w_old, self.b_old = w_old.clone(), b_old.clone()
        self.lin = torch.nn.Linear(w_old.shape[1], self.K + rows0.shape[0]).double()
        with torch.no_grad():
            self.lin.weight.copy_(torch.cat([w_old, rows0[:, :-1]]))
            self.lin.bias.copy_(torch.cat([b_old, rows0[:, -1]]))
        self.opt = torch.optim.AdamW(self.lin.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def step(self, act, targets):
        """One step on (act [B, F], targets [B]); returns the batch-mean NLL before it and the new rows' gradient [n, F + 1]."""
        act = torch.as_tensor(np.asarray(act, dtype=np.float64))
        self.opt.zero_grad()
        nlls = -torch.log_softmax(self.lin(act), dim=-1)[torch.arange(len(act)), torch.as_tensor(np.asarray(targets, dtype=np.int64))]
        loss = nlls.mean()
        loss.backward()
        grad = torch.cat([self.lin.weight.grad[self.K:], self.lin.bias.grad[self.K:, None]], dim=1).clone()
        self.opt.step()
        with torch.no_grad():
            self.lin.weight[:self.K].copy_(self.w_old)
            self.lin.bias[:self.K].copy_(self.b_old)
        return loss.item(), grad.numpy()

    def rows(self):
        return torch.cat([self.lin.weight.detach()[self.K:], self.lin.bias.detach()[self.K:, None]], dim=1).numpy().copy()


def ulps_f32(got, want64):
    """|got - float32(want64)| in units of the float32 spacing at float32(want64) (subnormal spacing below the normal range)."""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def rel_rms(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))
