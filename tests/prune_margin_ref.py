"""Numpy restatement of the per-query pruning margin (include/ripor_hip.h: rpr_search_margins) from the per-step taps of a
search: the logits, the child bitmap and the cumulative beam scores. Test infrastructure, never imported by the product.

At step t the candidates of a query are key[b, c] = ((float64)logit[b, c] + (valid[b, c] ? 0 : -1e9)) + score_before[b]
(the selection's keys; score_before = 0 for beam 0 and -1e9 for the others at step 0, then the previous step's slot
scores). Sorted descending, gap_t = key[B-1] - key[B] if key[B] > -1e8 else +inf; margin = min over the steps."""
import numpy as np

DEAD = -1e8   # candidates at or below this are masked tokens / dead beams (they carry -1e9): no competitors


def unpack_valid(words, B, V):
    """[..., B*V/64] 64-bit words (bit beam*V + token, little end first) -> bool [..., B, V]."""
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[:-1] + (B, V)).astype(bool)


def step_gaps(step_logits, step_valid, step_scores, B, Vreal=None):
    """step_logits [L, Q*B, V] float32 (the logits the selection ranked: log-softmax values where that applies),
    step_valid bool [L, Q, B, V], step_scores [L, Q, B] float64 after each step -> gaps [L, Q] float64.
    Vreal: columns Vreal..V-1 are padding of the logits rows, no candidates."""
    L, R, V = step_logits.shape
    Q = R // B
    Vr = V if Vreal is None else Vreal
    gaps = np.full((L, Q), np.inf)
    if B * Vr <= B:
        return gaps
    before = np.full((Q, B), -1e9)
    before[:, 0] = 0.0
    for t in range(L):
        lg = step_logits[t].reshape(Q, B, V)[:, :, :Vr].astype(np.float64)
        ok = np.asarray(step_valid[t]).reshape(Q, B, V)[:, :, :Vr]
        key = (lg + np.where(ok, 0.0, -1e9)) + before[:, :, None]
        srt = -np.sort(-key.reshape(Q, B * Vr), axis=1)
        gaps[t] = np.where(srt[:, B] > DEAD, srt[:, B - 1] - srt[:, B], np.inf)
        before = np.asarray(step_scores[t], dtype=np.float64).reshape(Q, B)
    return gaps


def prune_margin_ref(step_logits, step_valid, step_scores, B, Vreal=None):
    return step_gaps(step_logits, step_valid, step_scores, B, Vreal).min(axis=0)
