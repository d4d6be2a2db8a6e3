"""The outer loop of a batched Newton-CG solve (svm.fit_squared_hinge, logreg.fit): P independent convex problems advance together, their
scalars in a device state table whose columns 0-12 are hip.NCG_* (csrc/newton_cg.h). The loop owns the control flow and the one read-back per
Newton iteration; what the objective is, and which kernels and GEMMs evaluate it, arrives as callbacks that enqueue work and return nothing."""
from typing import Callable

import torch

from . import hip


def solve(state: torch.Tensor, begin: Callable[[], None], cg_update: Callable[[], None], grad: Callable[[], None],
          hess_vec: Callable[[], None], line_search: Callable[[], None], max_newton: int, max_cg: int, first_cap: int) -> int:
    """Run Newton iterations until no problem is active; returns the number of CG iterations enqueued (all problems advance together).
    A Newton iteration: grad() (the gradient at the current point), begin() (newton_begin: stopping test and CG start per problem), one
    read-back of `state`, then cap x (hess_vec() (H d of the CG direction), cg_update()) with no host synchronisation, then line_search()
    (which also moves the point). cap is first_cap in the first iteration and min(max_cg, max(10, 2 x the most CG iterations a still-active
    problem used in the previous one)) afterwards; a solve that hits it still gives a descent direction. At most max_newton + 1 gradients
    are evaluated: newton_begin stops a problem at max_newton, so the last pass only records the final gradients."""
    cap, launched = first_cap, 0
    for _ in range(max_newton + 1):
        grad()
        begin()
        st = state.cpu()                                            # the one read-back of this Newton iteration
        active = st[:, hip.NCG_ACTIVE] != 0
        if not bool(active.any()):
            break
        if launched:
            used = int(st[active, hip.NCG_CGLAST].max().item())
            cap = min(max_cg, max(10, 2 * used))
        for _ in range(cap):
            hess_vec()
            cg_update()
        launched += cap
        line_search()
    return launched
