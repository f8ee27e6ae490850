"""Whether Python hooks sit on modules: a fused kernel or a replayed graph
would skip them, so both fall back to the torch modules when one does."""

from __future__ import annotations


def hooked(*nets) -> bool:
    from torch.nn.modules import module as M

    if (M._global_forward_hooks or M._global_forward_pre_hooks or M._global_backward_hooks or
            getattr(M, "_global_backward_pre_hooks", None)):
        return True
    for net in nets:
        for m in net.modules():
            if (m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or
                    getattr(m, "_backward_pre_hooks", None)):
                return True
    return False
