"""DINO loss on the HIP kernels (mirror of adell_mri/modules/self_supervised/losses/dino.py).

``DinoLoss.forward(a, b)`` is ``-mean_r sum_k p_t[r, k] log_softmax(a / t1)[r, k]`` with the teacher
scores ``p_t = softmax((b - centers) / t2)`` ("center") or the Sinkhorn-Knopp assignment of
``exp(b / t2)`` ("sk"). The forward is one fused kernel family (csrc/dino.hip): a single pass over
``a`` and ``b``, rows split over workgroups, nothing of size [rows, n_features] saved for the
backward. Constructor, attributes and methods are the reference's.

Differences, on purpose:
  * the ``centers`` buffer keeps shape ``[n_features]``. The reference's turns ``[1, n_features]``
    after its first update (it adds a ``keepdim`` sum); the values are the same.
  * ``get_scores_teacher`` / ``get_log_scores_student`` return what the reference returns but carry
    no gradient: ``forward`` is the differentiable path and does not call them.
"""
import torch
import torch.distributed as dist

from .... import functional as HF
from .... import ops


class DinoLoss(torch.nn.Module):
    def __init__(self, temperatures: float | tuple[float, float], n_features: int,
                 center_m: float = 0.9, teacher_score_method: str = "center",
                 sk_iterations: int = 3):
        super().__init__()
        self.temperatures = temperatures
        self.n_features = n_features
        self.center_m = center_m
        self.teacher_score_method = teacher_score_method
        self.sk_iterations = sk_iterations
        assert self.teacher_score_method in ["center", "sk"]
        if isinstance(self.temperatures, float):
            self.temperatures = [self.temperatures, self.temperatures]
        self.t1 = self.temperatures[0]
        self.t2 = self.temperatures[1]
        self.register_buffer("centers", torch.zeros([self.n_features]))
        self.updated = True
        self.reduce_handle = None
        self.len_teacher_output = None
        self.async_batch_center = None

    @property
    def world_size(self) -> int:
        return dist.get_world_size() if dist.is_initialized() else 1

    @torch.no_grad()
    def apply_center_update(self) -> None:
        """The pending update, once: centers = centers * m + sum / (rows * world) * (1 - m)."""
        if self.updated is False:
            if self.async_batch_center is None:
                return
            if self.reduce_handle is not None:
                self.reduce_handle.wait()
                self.reduce_handle = None
            ops.dino_center_apply(self.centers, self.async_batch_center, self.center_m,
                                  self.len_teacher_output * self.world_size)
            self.updated = True

    @torch.no_grad()
    def update_centers(self, x: torch.Tensor) -> None:
        self.reduce_center_update(x)

    @torch.no_grad()
    def reduce_center_update(self, x: torch.Tensor) -> None:
        """Stores the column sum of ``x`` ([1, n_features]) and, when torch.distributed is
        initialised, starts its asynchronous all-reduce; applied lazily by the next
        ``get_scores_teacher`` / ``forward``."""
        self.updated = False
        if len(x.shape) > 2:
            x = x.flatten(end_dim=-2)
        self.len_teacher_output = len(x)
        self.async_batch_center = ops.dino_center_sum(x.detach())
        if dist.is_initialized():
            self.reduce_handle = dist.all_reduce(self.async_batch_center, async_op=True)

    @torch.no_grad()
    def get_scores_teacher(self, x: torch.Tensor) -> torch.Tensor:
        if self.teacher_score_method == "center":
            self.apply_center_update()
            return ops.dino_softmax(x.detach(), self.centers, self.t2)
        return self.sinkhorn_knopp_teacher(x)

    @torch.no_grad()
    def get_log_scores_student(self, x: torch.Tensor) -> torch.Tensor:
        return ops.dino_log_softmax(x.detach(), self.t1)

    @torch.no_grad()
    def sinkhorn_knopp_teacher(self, x: torch.Tensor) -> torch.Tensor:
        """[rows, n_features] assignment (fp32 whatever comes in, as the reference casts)."""
        x = x.detach().float().flatten(end_dim=-2)
        world = self.world_size
        reduce = dist.all_reduce if world > 1 else None
        return ops.dino_sk_scores(x, self.t2, self.sk_iterations, world_size=world, reduce=reduce)

    def forward(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if self.teacher_score_method == "center":
            self.apply_center_update()
            return HF.dino_loss(a, b, self.centers, self.t1, self.t2)
        # the assignment comes back as rows [R, n_features]; the student's rows go with it
        return HF.dino_loss(a.flatten(end_dim=-2), self.sinkhorn_knopp_teacher(b), None, self.t1,
                            self.t2, teacher_is_scores=True)
