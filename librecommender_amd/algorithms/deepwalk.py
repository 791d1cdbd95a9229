"""`DeepWalk` (`libreco/algorithms/deepwalk.py`): skip-gram over random walks on the item graph, with the reference's
constructor and checkpoints.  The reference trains with `gensim.Word2Vec(sg=1, hs=1, min_count=1)`, whose default
`negative=5` stays on: hierarchical softmax and 5 negatives.  Here the walks and the training run on the device
(bases/word2vec_base.py).

The graph is the reference's (`deepwalk.py:79-84`): items[i] -> items[i + 1] of every user list, duplicates kept as
multiplicity.  A pass over the corpus is `n_walks` rounds, each a permutation of the items drawn from one
`default_rng(seed)` as the reference draws them; a walk ends early at a node without successors.  The reference picks every
step with an unseeded `random.choice`, so it is not reproducible itself; here the step is mix64 of (seed, pass, walk, step).
Pass 0 gives the counts, passes 1 .. n_epochs are the training epochs."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..bases.word2vec_base import Word2VecBase


class DeepWalk(Word2VecBase):
    use_hs = True

    def __init__(self, task, data_info, embed_size=16, norm_embed=False, n_walks=10, walk_length=10, window_size=5,
                 n_epochs=10, n_threads=0, seed=42, lower_upper_bound=None, batch_size=256, device="cuda"):
        super().__init__(task, data_info, embed_size, norm_embed, window_size, n_epochs, n_threads, seed, lower_upper_bound,
                         batch_size, device)
        assert task == "ranking", "DeepWalk is only suitable for ranking"
        if walk_length < 1 or n_walks < 1:
            raise ValueError("`n_walks` and `walk_length` must be at least 1")
        self.all_args = locals()
        self.n_walks, self.walk_length = n_walks, walk_length
        self._succ = None
        self._passes = {}

    def successor_csr(self):
        """The reference's graph as a CSR over the items: the successors of a node in the order the user lists give them."""
        heads, tails = [], []
        for items in self.user_consumed.values():
            items = np.asarray(items, dtype=np.int64)
            heads.append(items[:-1])
            tails.append(items[1:])
        heads = np.concatenate(heads) if heads else np.zeros(0, dtype=np.int64)
        tails = np.concatenate(tails) if tails else np.zeros(0, dtype=np.int64)
        order = np.argsort(heads, kind="stable")
        ptr = np.zeros(self.n_items + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(np.bincount(heads, minlength=self.n_items))
        return ptr, tails[order].astype(np.int32)

    def _prepare_corpus(self):
        ptr, idx = self.successor_csr()
        self._succ = (torch.from_numpy(ptr).to(self.device), torch.from_numpy(idx).to(self.device))
        self._walk_rng = np.random.default_rng(self.seed)
        self._passes = {}

    def walk_starts(self, pass_no):
        """The start nodes of a pass: `n_walks` permutations of the items, consumed from one generator pass after pass."""
        while len(self._passes) <= pass_no:
            rounds = [self._walk_rng.permutation(self.n_items) for _ in range(self.n_walks)]
            self._passes[len(self._passes)] = np.concatenate(rounds).astype(np.int32)
        return self._passes[pass_no]

    def corpus(self, pass_no):
        starts = torch.from_numpy(self.walk_starts(pass_no)).to(self.device)
        walks, lens = ops.w2v_walks(starts, self._succ[0], self._succ[1], self.n_items, self.walk_length, self.seed, pass_no)
        tokens = walks[walks >= 0].contiguous()
        sptr = torch.nn.functional.pad(torch.cumsum(lens, 0, dtype=torch.int64), (1, 0))
        return tokens, sptr
