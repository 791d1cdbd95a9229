"""`ItemCF` (`libreco/algorithms/item_cf.py`): item-based collaborative filtering on the device (see `bases/cf_base.py`)."""
from ..bases import CfBase


class ItemCF(CfBase):
    def __init__(self, task, data_info, sim_type="cosine", k_sim=20, store_top_k=True, block_size=None, num_threads=1,
                 min_common=1, mode="invert", seed=42, lower_upper_bound=None):
        super().__init__(task, data_info, "item_cf", sim_type, k_sim, store_top_k, block_size, num_threads, min_common,
                         mode, seed, lower_upper_bound)
        self.all_args = locals()

    def _predict_rows(self):
        # `item_cf.py:70-115`: the first k_sim entries of the similarity row against the interacting items
        return "user", False

    def rebuild_model(self, path, model_name, **kwargs):
        raise NotImplementedError("`ItemCF` doesn't support model retraining")
