"""The teacher's side of a distillation step: the temperature KL loss on its logits.

kotoba-whisper's ``train_step`` (run_distillation.py:625-661) runs the frozen teacher without gradients, then

    teacher_distribution = softmax(teacher.logits / T)
    student_distribution = log_softmax(student.logits / T)
    kl = kl_divergence(teacher_distribution, student_distribution, labels) * T**2        (:614-622, :652-657)

where ``kl_divergence`` is ``KLDivLoss(reduction="none")`` summed over every position whose label is >= 0 and divided
by the number of such positions.  ``kd_loss`` is that expression as one device op (``kw_kd_loss``, csrc/kd.hip): it
reads both logit tensors twice, keeps nothing of size [B, T, V] besides the student's gradient, and is differentiable
in the student's logits only -- the teacher is frozen.

    teacher_out = teacher(**batch)                       # KWhisperForConditionalGeneration.forward, no grad
    kl = kd_loss(student_out.logits, teacher_out.logits, batch["labels"], temperature)
"""
from __future__ import annotations

import torch

from . import ops


def _rows(x: torch.Tensor, V: int) -> torch.Tensor:
    """``x`` [..., V] as an [N][V] view with one row stride and a unit inner stride; a copy only when there is no
    such view (a strided view of whole rows stays a view)."""
    if x.stride(-1) != 1:
        x = x.contiguous()
    if x.dim() == 2:
        return x
    try:
        return x.view(-1, V)
    except RuntimeError:
        return x.reshape(-1, V)


class _KDLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, labels, temperature):
        V = student.shape[-1]
        s2, t2 = _rows(student.detach(), V), _rows(teacher, V)
        lab = labels.reshape(-1).to(device=s2.device, dtype=torch.int64).contiguous()
        # (the gradient is made with the forward: the kernel's second pass has p and q in registers anyway)
        # a student that asks for no gradient (an evaluation step) gets the forward-only launch
        grad = torch.empty((s2.shape[0], V), device=s2.device, dtype=s2.dtype) if ctx.needs_input_grad[0] else None
        loss, row_kl = ops.kd_loss(t2, s2, lab, temperature, grad=grad)
        ctx.save_for_backward(grad)
        ctx.shape = student.shape
        ctx.mark_non_differentiable(row_kl)
        return loss.reshape(()), row_kl

    @staticmethod
    def backward(ctx, grad_loss, _grad_rows):
        (grad,) = ctx.saved_tensors
        # (the 0-d f32 weight multiplies as it is: a bf16 gradient is rounded once, the weight never)
        return (grad * grad_loss).view(ctx.shape), None, None, None


def kd_loss(student_logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor,
            temperature: float = 2.0, return_row_kl: bool = False):
    """``kl_divergence(softmax(t / T), log_softmax(s / T), labels) * T**2`` of the reference's ``train_step`` as a 0-d
    f32 device tensor, differentiable in ``student_logits``.

    ``student_logits`` / ``teacher_logits``: [B, T, V] or [N, V] device tensors of one shape (strided views of whole
    rows are taken as they are); the student f32 or bf16, the teacher detached and cast to f32 if it is not.
    ``labels``: the integer labels of the same leading shape; a negative label (-100) leaves its position out.
    With no valid position the loss is NaN, as the reference's 0 / 0, and the gradient zero.
    ``return_row_kl``: also return the per-position divergences (f32, flattened; no gradient flows through them)."""
    if not (isinstance(student_logits, torch.Tensor) and isinstance(teacher_logits, torch.Tensor)):
        raise TypeError("kd_loss takes tensors")
    if not student_logits.is_cuda or not teacher_logits.is_cuda:
        raise ValueError("kd_loss: kwhisper ops take device (cuda) tensors")
    if student_logits.shape != teacher_logits.shape or student_logits.dim() not in (2, 3):
        raise ValueError("kd_loss: student_logits and teacher_logits must share one [B, T, V] or [N, V] shape")
    if tuple(labels.shape) != tuple(student_logits.shape[:-1]):
        raise ValueError("kd_loss: labels must have the logits' leading shape")
    if student_logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("kd_loss: student_logits must be float32 or bfloat16")
    if not float(temperature) > 0.0 or float(temperature) == float("inf"):
        raise ValueError("kd_loss: temperature must be a finite float > 0")
    teacher = teacher_logits.detach()
    if teacher.dtype != torch.float32:
        teacher = teacher.float()
    loss, row_kl = _KDLoss.apply(student_logits, teacher, labels, float(temperature))
    return (loss, row_kl) if return_row_kl else loss
