"""A numpy float32 restatement of `vqvs_speaker_mix` (include/vqvs.h): products and sums in slot order, each rounded to float32 on its
own, the first used slot's product the initial value.  numpy's float32 arithmetic rounds every operation, so there is nothing to
contract: the kernel has to give these bits."""
import numpy as np


def mix_ref(table: np.ndarray, idx: np.ndarray, w: np.ndarray) -> np.ndarray:
    """table [K, E] float32, idx [B, J] int (negative: unused slot; >= K reads row K - 1), w [B, J] float32 -> out [B, E] float32."""
    table, w = np.asarray(table, dtype=np.float32), np.asarray(w, dtype=np.float32)
    K, E = table.shape
    B, J = idx.shape
    out = np.zeros((B, E), dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for b in range(B):
            acc = None
            for j in range(J):
                if idx[b, j] < 0:
                    continue
                prod = (w[b, j] * table[min(int(idx[b, j]), K - 1)]).astype(np.float32)
                acc = prod if acc is None else (acc + prod).astype(np.float32)
            if acc is not None:
                out[b] = acc
    return out


def mix_case(K: int, E: int, B: int, J: int, seed: int, unused: str = "some"):
    """(table, idx, w): table elements N(0, 1) times 1e-30, 1 or 1e30, one magnitude per element; weights N(0, 1); `unused` "none",
    "some" (each slot unused with probability 1/4; row 0 keeps its first slot unused and, with J >= 3, a middle one) or "all" (row 0
    has no used slot at all)."""
    rng = np.random.RandomState(seed)
    table = (rng.randn(K, E) * np.array([1e-30, 1.0, 1e30])[rng.randint(0, 3, (K, E))]).astype(np.float32)
    idx = rng.randint(0, K, (B, J)).astype(np.int32)
    w = rng.randn(B, J).astype(np.float32)
    if unused != "none":
        idx[rng.rand(B, J) < 0.25] = -1
        idx[0, 0] = -1
        if J >= 3:
            idx[0, J // 2] = -1
            idx[0, J - 1] = K - 1
    if unused == "all":
        idx[0, :] = -1
    return table, idx, w
