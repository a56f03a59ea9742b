"""hybridflux.flat on CPU tensors: flat_view only compares storages, so the
helpers the trainers share are exercised fully without a device."""
import pytest
import torch

CPU = torch.device("cpu")


def _models():
    from hybridflux import PINN, FluxGNN, PureGNN
    torch.manual_seed(0)
    return [FluxGNN(4, 8, 1), PureGNN(4, 8, 1), PINN(6, 8, 2)]


@pytest.fixture(params=range(3), ids=["FluxGNN", "PureGNN", "PINN"])
def model(request):
    return _models()[request.param]


def test_unflattened_is_a_copy(model):
    from hybridflux.flat import flat_params, flat_view
    params = list(model.parameters())
    assert flat_view(params, CPU) is None
    flat, home = flat_params(params, CPU)
    assert home is False and flat.dtype == torch.float32 and not flat.requires_grad
    assert torch.equal(flat, torch.cat([v.reshape(-1) for v in model.state_dict().values()]))
    assert flat.untyped_storage().data_ptr() != params[0].untyped_storage().data_ptr()


def test_flatten_makes_one_buffer_and_keeps_the_parameters(model):
    from hybridflux.flat import flat_params, flat_view
    params = list(model.parameters())
    ids = [id(q) for q in params]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.flatten_parameters_() is model
    params = list(model.parameters())
    assert [id(q) for q in params] == ids
    after = model.state_dict()
    assert list(after) == list(before)
    assert all(after[k].shape == before[k].shape and torch.equal(after[k], before[k]) for k in before)
    flat = flat_view(params, CPU)
    assert flat is not None and flat.dim() == 1 and flat.numel() == sum(q.numel() for q in params)
    assert torch.equal(flat, torch.cat([v.reshape(-1) for v in before.values()]))
    flat[0] = 12345.0  # a view: the write lands in the first parameter
    assert params[0].detach().reshape(-1)[0].item() == 12345.0
    same, home = flat_params(params, CPU)
    assert home is True and same.data_ptr() == flat.data_ptr() and same.numel() == flat.numel()


@pytest.mark.parametrize("how", ["replaced", "swapped", "float64"])
def test_flat_view_notices_a_broken_buffer(model, how):
    from hybridflux.flat import flat_params, flat_view
    model.flatten_parameters_()
    params = list(model.parameters())
    assert flat_view(params, CPU) is not None
    if how == "replaced":
        params[1] = params[1].detach().clone()
    elif how == "swapped":
        params[0], params[1] = params[1], params[0]
    else:
        params[-1] = params[-1].detach().double()
    assert flat_view(params, CPU) is None
    flat, home = flat_params(params, CPU)
    assert home is False and flat.dtype == torch.float32
    assert torch.equal(flat, torch.cat([q.detach().reshape(-1).float() for q in params]))


def test_split_and_assign_round_trip(model):
    from hybridflux.flat import assign_grads, flat_view, split_flat
    params = list(model.parameters())
    P = sum(q.numel() for q in params)
    gp = torch.arange(P, dtype=torch.float32)
    pieces = split_flat(gp, [q.shape for q in params], [q.device for q in params])
    assert [g.shape for g in pieces] == [q.shape for q in params]
    assert all(g.untyped_storage().data_ptr() == gp.untyped_storage().data_ptr() for g in pieces)  # cut, not copied
    assert torch.equal(torch.cat([g.reshape(-1) for g in pieces]), gp)
    for home in (True, False):
        for q in params:
            q.grad = None
        assign_grads(params, gp, home)
        grads = [q.grad for q in params]
        assert [g.shape for g in grads] == [q.shape for q in params]
        view = flat_view(grads, CPU)  # what FlatAdam reads instead of concatenating
        assert view is not None and view.data_ptr() == gp.data_ptr() and torch.equal(view, gp)


def test_drives_exactly(model):
    from hybridflux.flat import drives_exactly
    params = list(model.parameters())
    assert drives_exactly(torch.optim.SGD(model.parameters(), lr=0.1), params)
    two = torch.optim.SGD([{"params": params[:1]}, {"params": params[1:]}], lr=0.1)
    assert not drives_exactly(two, params)
    assert not drives_exactly(torch.optim.SGD(params[:-1], lr=0.1), params)
    assert not drives_exactly(torch.optim.SGD(params[::-1], lr=0.1), params)  # the same set, another order
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    params[-1].requires_grad_(False)
    assert not drives_exactly(opt, params)


def test_flatten_drops_fluxgnn_packed_copies():
    """FluxGNN.flatten_parameters_ also forgets its packed inference weights
    (they point at the old storages)."""
    model = _models()[0]

    class Packed:
        closed = False

        def close(self):
            self.closed = True

    dm = Packed()
    model._packed["cpu"] = (None, dm)
    model.flatten_parameters_()
    assert dm.closed and model._packed == {}
