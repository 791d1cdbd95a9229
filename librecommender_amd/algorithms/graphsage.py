"""`GraphSage` (`libreco/algorithms/graphsage.py`, the non-DGL model): same constructor and checks; sampling and the tower on the
device (`SageBase`, nets/sage_net.py, csrc/sage.hip).  `fused=False` runs the tower composed from torch ops instead."""
from __future__ import annotations

from ..bases.sage_base import SageBase


class GraphSage(SageBase):
    def __init__(self, task, data_info, loss_type="cross_entropy", paradigm="i2i", embed_size=16, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-8, amsgrad=False, reg=None, batch_size=256, num_neg=1, dropout_rate=0.0,
                 remove_edges=False, num_layers=2, num_neighbors=3, num_walks=10, sample_walk_len=5, margin=1.0,
                 sampler="random", start_node="random", focus_start=False, seed=42, device="cuda", lower_upper_bound=None,
                 fused=True):
        super().__init__(task, data_info, loss_type, paradigm, embed_size, n_epochs, lr, lr_decay, epsilon, amsgrad, reg,
                         batch_size, num_neg, dropout_rate, remove_edges, num_layers, num_neighbors, num_walks,
                         sample_walk_len, margin, sampler, start_node, focus_start, seed, device, lower_upper_bound,
                         fused=fused)
        self.all_args = locals()
