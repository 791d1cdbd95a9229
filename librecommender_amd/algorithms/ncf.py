"""`NCF` (`libreco/algorithms/ncf.py`, He et al., "Neural Collaborative Filtering"): the reference's constructor and checks over
`FeatBase`'s `fit / predict / recommend_user / save / load / rebuild_model`.  The net is `nets/ncf_net.py` on csrc/ncf.hip (the
exact GMF product with the gather, the join of the GMF gradient with the MLP's row gradient, the inference tower in one launch);
full-catalogue ranking is `recommendation/ncf_catalog.py`.  Feature columns of a `DatasetFeat` are ignored, as in the reference.

Deliberate differences from the reference:
  (a) the default optimiser of both embedding variables is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the
      reference's TF1 semantics (every row decays and moves every step), and `reg` selects it;
  (b) `tf_sess_config` is accepted and ignored; under a process group of more than one rank `fit` raises;
  (c) `save_tf_variables` / `load_tf_variables` raise: NCF's graph-variable names are not mapped.
"""
from __future__ import annotations

from ..bases.base import hip_device
from ..nets.ncf_net import NCFNet
from ..utils.validate import hidden_units_config
from .fm import _FMCommon


class NCF(_FMCommon):
    def __init__(self, task, data_info, loss_type="cross_entropy", embed_size=16, n_epochs=20, lr=0.01, lr_decay=False,
                 epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, use_bn=True, dropout_rate=None,
                 hidden_units=(128, 64, 32), seed=42, lower_upper_bound=None, tf_sess_config=None, device="cuda",
                 dense_adam=False):
        super().__init__(task, data_info, lower_upper_bound)
        self.all_args = locals()
        self._common(data_info, loss_type, embed_size, n_epochs, lr, lr_decay, epsilon, reg, batch_size, sampler, num_neg,
                     use_bn, dropout_rate, "normal", seed, device, dense_adam)
        self.hidden_units = hidden_units_config(hidden_units)

    def build_model(self):
        self.device = hip_device(self._device_arg)
        self.net = NCFNet(self.n_users, self.n_items, self.embed_size, self.hidden_units, self.use_bn, self.dropout_rate,
                          self.lr, self.epsilon, self.seed, self.device, self.dense_adam, self.reg)

    def _catalog_scorer(self):
        sc = getattr(self, "_scorer", None)
        if sc is None or sc.net is not self.net:
            from ..recommendation.ncf_catalog import NCFCatalogScorer

            sc = self._scorer = NCFCatalogScorer(self)
        return sc

    def save_tf_variables(self, path, model_name):
        raise NotImplementedError("NCF: the reference's graph-variable names are not mapped")

    def load_tf_variables(self, path, model_name):
        raise NotImplementedError("NCF: the reference's graph-variable names are not mapped")
