"""`PinSage` (`libreco/algorithms/pinsage.py`, the non-DGL model): same constructor and checks; the importance-walk neighbour
sampling and the tower on the device (`SageBase`, nets/pinsage_net.py, csrc/pinsage.hip).  `fused=False` runs
the tower composed from torch ops instead.  `remove_edges` takes effect for i2i training only, as in the reference."""
from __future__ import annotations

from ..bases.sage_base import SageBase


class PinSage(SageBase):
    def __init__(self, task, data_info, loss_type="max_margin", paradigm="i2i", embed_size=16, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-8, amsgrad=False, reg=None, batch_size=256, num_neg=1, dropout_rate=0.0,
                 remove_edges=False, num_layers=2, num_neighbors=3, num_walks=10, neighbor_walk_len=2, sample_walk_len=5,
                 termination_prob=0.5, margin=1.0, sampler="random", start_node="random", focus_start=False, seed=42,
                 device="cuda", lower_upper_bound=None, fused=True):
        self.neighbor_walk_len, self.termination_prob = neighbor_walk_len, termination_prob
        super().__init__(task, data_info, loss_type, paradigm, embed_size, n_epochs, lr, lr_decay, epsilon, amsgrad, reg,
                         batch_size, num_neg, dropout_rate, remove_edges, num_layers, num_neighbors, num_walks,
                         sample_walk_len, margin, sampler, start_node, focus_start, seed, device, lower_upper_bound,
                         fused=fused)
        self.all_args = locals()

    def net_class(self):
        from ..nets.pinsage_net import PinSageNet

        # what the device sampler serves: at most 64 visits per node
        if not (self.num_walks >= 1 and self.neighbor_walk_len >= 1 and self.num_walks * self.neighbor_walk_len <= 64):
            raise ValueError(f"{self.model_name}: `num_walks` and `neighbor_walk_len` must be at least 1 and their product at "
                             f"most 64 (the device sampler's range), got {self.num_walks} and {self.neighbor_walk_len}")
        if not self.termination_prob == self.termination_prob:
            raise ValueError(f"{self.model_name}: `termination_prob` must be a number")
        return PinSageNet, dict(num_walks=self.num_walks, neighbor_walk_len=self.neighbor_walk_len,
                                termination_prob=self.termination_prob,
                                remove_edges=bool(self.remove_edges) and self.paradigm == "i2i")
