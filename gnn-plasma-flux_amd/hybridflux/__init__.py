"""hybridflux — MI355X-native hybrid rollout engine for the hot path of
shanedirksen/gnn-plasma-flux.  Same public surface as the reference package
(src/__init__.py:4-26): BaselineSolver, FluxGNN, HybridSolver,
build_chain_graph and the config dictionaries; plus batched device entry
points (step_batch / run_batch), HybridEnsemble (a set of checkpoints rolled
out in one launch), the engine module and the multi-GPU IC-sharded rollout
driver, and FineReference (the classical solver on a refined grid with
substeps, coarse-grained onto the training grid in one launch: the data and
the score behind the reference README's fine-baseline claims), and
StateNoise (seeded Gaussian noise on a training step's start state, drawn on
the device; the K-step trainers' noise= option).
"""
from .baseline_solver import BaselineSolver
from .baselines import PINN, PureGNN
from .config import ABLATION_CONFIGS, DATASET_CONFIG, EVAL_CONFIG, MODEL_CONFIG, STENCIL_RADII, TRAIN_CONFIG
from .fine_reference import FineReference
from .flux_gnn import FluxGNN
from .graph_constructor import build_chain_graph, build_chain_graph_batch, chain_edge_index
from .hybrid_solver import HybridEnsemble, HybridSolver
from .training import StateNoise

__all__ = [
    "BaselineSolver",
    "FineReference",
    "PureGNN",
    "PINN",
    "FluxGNN",
    "HybridSolver",
    "HybridEnsemble",
    "StateNoise",
    "build_chain_graph",
    "build_chain_graph_batch",
    "chain_edge_index",
    "DATASET_CONFIG",
    "MODEL_CONFIG",
    "TRAIN_CONFIG",
    "STENCIL_RADII",
    "ABLATION_CONFIGS",
    "EVAL_CONFIG",
]
