"""Flat-parameter helpers shared by the models and the trainers.

The training kernels read a model's parameters as one float32 buffer in
state-dict order and return the gradient as one such buffer.  This module is
the one place that turns a parameter list into that buffer and the gradient
buffer back into per-parameter pieces.  It imports only torch.
"""
import torch


def flat_view(params, dev):
    """The parameters as one flat float32 tensor, without a copy, when they are
    consecutive contiguous pieces of one device buffer (after
    flatten_parameters_); otherwise None."""
    p0 = params[0]
    base, off, n = p0.untyped_storage().data_ptr(), p0.storage_offset(), 0
    for q in params:
        if (q.device != dev or q.dtype != torch.float32 or not q.is_contiguous()
                or q.untyped_storage().data_ptr() != base or q.storage_offset() != off + n):
            return None
        n += q.numel()
    return p0.detach().as_strided((n,), (1,), off)


def flat_params(params, dev):
    """(flat, home): the parameters as one flat float32 tensor on dev -- the
    view of their one buffer when there is one (home True: the kernels read
    the parameters in place), otherwise a detached concatenated copy."""
    flat = flat_view(params, dev)
    if flat is not None:
        return flat, True
    return torch.cat([q.detach().reshape(-1).to(device=dev, dtype=torch.float32) for q in params]), False


def split_flat(gp, shapes, devices):
    """The flat gradient gp cut into one piece per parameter, each a view of gp
    reshaped to the parameter's shape and moved to its device (for a piece
    already there .to returns the same tensor: no copy, no launch)."""
    grads, o = [], 0
    for shp, dev in zip(shapes, devices):
        n = shp.numel()
        grads.append(gp[o:o + n].view(shp).to(dev))
        o += n
    return grads


def assign_grads(params, gp, home=True):
    """q.grad = q's piece of the flat gradient gp, for every parameter (what
    backward() would leave, as views of one buffer).  home: gp lies on the
    parameters' own device (they were read in place); otherwise every piece is
    moved to its parameter's."""
    o = 0
    for q in params:
        g = gp[o:o + q.numel()].view_as(q)
        q.grad = g if home else g.to(q.device)
        o += q.numel()


def flatten_(module):
    """Re-home every parameter of module into one contiguous float32 buffer in
    state-dict order; the parameters keep their identity.  Returns module."""
    params = list(module.parameters())
    flat = torch.cat([q.detach().reshape(-1).to(torch.float32) for q in params])
    o = 0
    with torch.no_grad():
        for q in params:
            q.data = flat[o:o + q.numel()].view(q.shape)
            o += q.numel()
    return module


def drives_exactly(opt, params):
    """The optimizer drives exactly these parameters: one param group holding
    these parameter objects in this order, all of them requiring grad."""
    return (len(opt.param_groups) == 1 and [id(q) for q in opt.param_groups[0]["params"]] == [id(q) for q in params]
            and all(q.requires_grad for q in params))
