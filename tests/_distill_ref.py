"""Plain float64 restatements for the distillation tests: the temperature KL of kotoba-whisper's ``train_step`` and
HF's label shift, written out from their definitions (numpy only)."""
import numpy as np


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def kd_ref(teacher, student, labels, T):
    """(loss, row_kl [N], grad [N][V]) in float64.  teacher / student: [N][V] (any float dtype numpy can widen),
    labels [N].  row_kl = sum_v p (log p - log q) with p = softmax(teacher / T), q = softmax(student / T), a term with
    p == 0 counting 0; rows with a negative label count nothing; loss = T^2 sum(row_kl) / n_valid (NaN for
    n_valid == 0); grad = d loss / d student = T (q - p) / n_valid, zero on ignored rows."""
    T = float(T)
    lp = log_softmax64(np.asarray(teacher, np.float64) / T)
    lq = log_softmax64(np.asarray(student, np.float64) / T)
    p, q = np.exp(lp), np.exp(lq)
    with np.errstate(invalid="ignore"):
        terms = np.where(p > 0, p * (lp - lq), 0.0)
    valid = np.asarray(labels).reshape(-1) >= 0
    row = np.where(valid, terms.sum(-1), 0.0)
    n = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(T * T) * row.sum() / np.float64(n)
    grad = np.zeros_like(p)
    if n:
        grad[valid] = T * (q[valid] - p[valid]) / n
    return loss, row, grad


def shift_right(labels, pad_id, start_id):
    """decoder_input_ids from labels: one step to the right behind ``start_id``, -100 replaced by ``pad_id``."""
    labels = np.asarray(labels, np.int64)
    out = np.empty_like(labels)
    out[:, 0] = start_id
    out[:, 1:] = labels[:, :-1]
    out[out == -100] = pad_id
    return out


def cross_entropy64(logits, labels):
    """Mean over the positions with a label >= 0 of -log_softmax(logits)[label] (HF's CrossEntropyLoss())."""
    lp = log_softmax64(logits).reshape(-1, np.asarray(logits).shape[-1])
    lab = np.asarray(labels).reshape(-1)
    v = lab >= 0
    return float(-lp[np.nonzero(v)[0], lab[v]].mean())
