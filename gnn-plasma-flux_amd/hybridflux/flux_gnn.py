"""FluxGNN with the reference's module tree and forward signature
(src/flux_gnn.py:6-67), executed by the MI355X kernels of libhybridflux.

The nn.Module layout (input_mlp / update_mlps / edge_mlp Sequentials) is kept
so reference checkpoints load with `load_state_dict` unchanged.  forward()
never runs these Linear layers itself: the parameters are packed (once per
change) into a device weight handle and the edge fluxes come from
  * the fused chain kernel (hf_chain_flux: chain_f32.hip / chain_k32.hip /
    chain_bf16.hip) when edge_index is a periodic chain — tagged by
    graph_constructor, or recognised by content — and the model has
    MODEL_CONFIG's width (in 4, hidden 128);
  * the generic-graph kernels (graph.hip) for any other edge_index
    (examples/smoke_test.py:53 passes a random one) or width.  A radius-R
    chain graph (graph_constructor.chain_edge_index(radius=R), R > 1) is such
    a graph: forward() returns all its 2*R*nx fluxes per IC, the reference's
    semantics on that edge list.  For a tagged (unmodified) radius graph and a
    model of MODEL_CONFIG's width in f32 the no-grad forward keeps the fused
    radius kernels' arithmetic (hf_graph_flux_radius: neighbour sums times
    W_b / (2R), one rounding per weight) so that the module and the solver
    share one definition; an untagged copy, and the forward under autograd,
    form the reference's float32 mean (sum / degree), the same bits for R <= 2
    and a rounding apart for R = 3.  The fused radius kernels compute only the
    first 2*nx fluxes and are reached through HybridSolver(graph_radius=R).

Host (CPU) tensors and a CPU-resident module — the reference's own call
pattern (examples/smoke_test.py:50-56, src/flux_gnn.py:40-67: the flux comes
back on the caller's device) — are staged to the current HIP device, computed
by the same kernels and copied back; gradients land on the parameters' and the
node features' own devices.  There is no CPU compute path: with no HIP device
visible a call raises.

Under autograd (grad enabled and a parameter or the node features requiring
grad) forward() runs the training kernels instead: the forward keeps an
activation tape on the device and backward() runs the HIP backward kernels
(hf_graph_backward: the chain-layout MFMA GEMMs of train_chain.hip on tagged
chains, the generic-graph kernels of graph.hip otherwise), so `loss.backward()`
in the reference trainer (scripts/training/train_ablation.py:203-205) works
unchanged.
"""
import torch
import torch.nn as nn

from . import engine
from .flat import flat_params, flatten_, split_flat
from .graph_constructor import chain_tag, chain_tag_radius, shared_chain_edge_index


class _TrainForward(torch.autograd.Function):
    """FluxGNN.forward with HIP backward kernels (parameter order = state dict)."""

    @staticmethod
    def forward(ctx, node_features, edge_index, dims, *params):
        dev = engine.compute_device(node_features, "node_features")
        flat, _ = flat_params(params, dev)
        flux, tape, nf, ei, chain_nx = engine.graph_forward_train(flat, dims, node_features.detach().to(dev),
                                                                  edge_index)
        ctx.save_for_backward(flat, tape, nf, ei)
        ctx.dims = dims
        ctx.chain_nx = chain_nx
        ctx.shapes = [q.shape for q in params]
        ctx.param_devices = [q.device for q in params]
        ctx.nf_dtype, ctx.nf_device = node_features.dtype, node_features.device
        return flux.to(node_features.device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_flux):
        flat, tape, nf, ei = ctx.saved_tensors
        gp, gnf = engine.graph_backward(flat, ctx.dims, nf, ei, ctx.chain_nx, tape, grad_flux,
                                        ctx.needs_input_grad[0])
        gnf = gnf.to(device=ctx.nf_device, dtype=ctx.nf_dtype) if gnf is not None else None
        return (gnf, None, None, *split_flat(gp, ctx.shapes, ctx.param_devices))


class FluxGNN(nn.Module):
    """Message-passing GNN predicting one flux per directed edge."""

    def __init__(self, input_dim=2, hidden_dim=32, num_layers=2, precision="f32"):
        super().__init__()
        self.precision = precision  # chain-kernel arithmetic: "f32" | "f16x3" | "bf16" (engine.DeviceModel)
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        self.input_mlp = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.ReLU())
        self.update_mlps = nn.ModuleList(
            [nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU()) for _ in range(num_layers)])
        self.edge_mlp = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                      nn.Linear(hidden_dim, 1))
        self._packed = {}

    # -- weights -------------------------------------------------------------
    def _signature(self):
        return (self.precision,) + tuple((p.data_ptr(), p._version, str(p.device)) for p in self.parameters())

    def device_model(self, device, radius=1):
        """The packed libhybridflux weight handle for `device` (rebuilt when any
        parameter changes).  radius: the stencil radius of the fused chain
        kernels (engine.DeviceModel); forward() itself always asks for 1, the
        ±1 chain its tagged graphs are, and HybridSolver(graph_radius=R) for R."""
        device = torch.device(device)
        key = str(device) if radius == 1 else f"{device}/r{int(radius)}"
        sig = self._signature()
        hit = self._packed.get(key)
        if hit is None or hit[0] != sig:
            if hit is not None:
                hit[1].close()
            sd = {k: v for k, v in self.state_dict().items()}
            self._packed[key] = (sig, engine.DeviceModel(sd, device, self.precision, radius))
        return self._packed[key][1]

    def flatten_parameters_(self):
        """Re-home every parameter into one contiguous float32 buffer in
        state-dict order (the parameters keep their identity, so an optimizer
        made before still holds them): the training forward then hands the
        kernels that buffer instead of concatenating the parameters each step.
        .to() / .cuda() afterwards undo it (the forward falls back to the copy)."""
        flatten_(self)
        for _, (_, dm) in list(self._packed.items()):
            dm.close()
        self._packed = {}
        return self

    def _apply(self, fn, *args, **kwargs):  # .to()/.cuda() invalidate packed copies
        out = super()._apply(fn, *args, **kwargs)
        for _, (_, dm) in list(self._packed.items()):
            dm.close()
        self._packed = {}
        return out

    # -- forward -------------------------------------------------------------
    @staticmethod
    def _chain_geometry(node_features, edge_index):
        N = node_features.shape[0]
        tag = chain_tag(edge_index)
        if tag is not None:
            B, nx = tag
            return (B, nx) if B * nx == N else None
        if edge_index.dim() == 2 and edge_index.shape[0] == 2 and edge_index.shape[1] == 2 * N and N > 0:
            ref = shared_chain_edge_index(N, 1, edge_index.device)
            if torch.equal(edge_index.to(torch.long), ref):
                return 1, N
        return None

    def forward(self, node_features, edge_index):
        """node_features [N, input_dim] float32, edge_index [2, E] int64 -> flux [E]
        on node_features' device (host inputs are computed on the current HIP
        device and the flux copied back)."""
        dev = engine.compute_device(node_features, "node_features")
        params = list(self.parameters())
        if torch.is_grad_enabled() and (node_features.requires_grad or any(q.requires_grad for q in params)):
            dims = (self.input_dim, self.hidden_dim, self.num_layers)
            return _TrainForward.apply(node_features, edge_index, dims, *params)
        dm = self.device_model(dev)
        geom = self._chain_geometry(node_features, edge_index)
        nf = node_features.to(device=dev, dtype=torch.float32)
        rtag = chain_tag_radius(edge_index) if geom is None else None
        if geom is not None and dm.chain_ok:
            flux = engine.chain_flux(dm, nf, geom[0], geom[1])
        elif (rtag is not None and rtag[2] > 1 and rtag[0] * rtag[1] == nf.shape[0] and dm.chain_ok
              and self.precision == "f32" and self.num_layers <= 8):
            # a tagged radius graph: every edge's flux, in the fused radius kernels' arithmetic
            flux = engine.graph_flux_radius(self.device_model(dev, rtag[2]), nf, edge_index, rtag[0], rtag[1])
        else:
            flux = engine.graph_flux(dm, nf, edge_index)
        return flux.to(node_features.device)
