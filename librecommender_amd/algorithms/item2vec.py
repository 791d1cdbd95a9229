"""`Item2Vec` (`libreco/algorithms/item2vec.py`): skip-gram with 5 negatives over every user's consumed list, with the
reference's constructor and checkpoints.  The reference trains with `gensim.Word2Vec(sg=1, hs=0, negative=5, min_count=1)`
on CPU threads; here the training runs on the device in windows of `batch_size` pairs (bases/word2vec_base.py, DESIGN.md
§7.9).  The corpus is the same in every pass: the consumed lists in `user_consumed` order."""
from __future__ import annotations

import torch

from ..bases.word2vec_base import Word2VecBase, flatten_lists


class Item2Vec(Word2VecBase):
    use_hs = False

    def __init__(self, task, data_info=None, embed_size=16, norm_embed=False, window_size=5, n_epochs=10, n_threads=0,
                 seed=42, lower_upper_bound=None, batch_size=256, device="cuda"):
        super().__init__(task, data_info, embed_size, norm_embed, window_size, n_epochs, n_threads, seed, lower_upper_bound,
                         batch_size, device)
        assert task == "ranking", "Item2Vec is only suitable for ranking"
        self.all_args = locals()
        self._corpus = None

    def corpus(self, pass_no):
        if self._corpus is None:
            tokens, sptr = flatten_lists(list(self.user_consumed.values()))
            self._corpus = (torch.from_numpy(tokens).to(self.device), torch.from_numpy(sptr).to(self.device))
        return self._corpus
