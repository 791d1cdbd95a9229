"""`RsItemCF` (`libreco/algorithms/item_cf_rs.py`): item-based collaborative filtering that can be retrained on new
interactions alone, on the device (see `bases/cf_base_rs.py`)."""
from ..bases import RsCfBase


class RsItemCF(RsCfBase):
    _cf_type = "item_cf"

    def __init__(self, task, data_info, k_sim=20, num_threads=1, min_common=1, mode="invert", seed=42,
                 lower_upper_bound=None):
        super().__init__(task, data_info, k_sim, num_threads, min_common, mode, seed, lower_upper_bound)
        self.all_args = locals()
