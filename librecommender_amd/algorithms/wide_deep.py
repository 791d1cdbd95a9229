"""`WideDeep` (`libreco/algorithms/wide_deep.py`, Cheng et al., "Wide & Deep Learning for Recommender Systems"): the
reference's constructor and checks over `FeatBase`'s `fit / predict / recommend_user / save / load / rebuild_model`.  The wide
side trains with FTRL-proximal on csrc/ftrl.hip, the deep side with Adam (`nets/wide_deep_net.py`); full-catalogue scoring is
the chunked forward.

Deliberate differences from the reference:
  (a) the deep side's default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1
      semantics, and `reg` selects it.  The wide tables move on the touched rows as in the reference (FTRL keeps no decaying
      moments, so its sparse apply already is row-wise); under `reg` every wide row moves every step, as in the reference;
  (b) sqrt(new_accum) - sqrt(accum) of the FTRL update is formed as g*g / (sqrt(new_accum) + sqrt(accum)), the same quantity
      without the f32 cancellation;
  (c) the FTRL slots are saved under the names of the Adam moments they replace (`opt::lin_m` = accumulator, `opt::lin_v` =
      linear, and the wide range of `opt::dense_m / opt::dense_v`);
  (d) `tf_sess_config` is accepted and ignored; under a process group of more than one rank `fit` raises;
      `save_tf_variables` / `load_tf_variables` raise: the `*_wide_var` / `*_deep_var` names are not mapped.
"""
from __future__ import annotations

from ..bases.base import hip_device
from ..nets.wide_deep_net import DEFAULT_LR, WideDeepNet
from ..utils.validate import hidden_units_config
from .fm import _FMCommon


def check_lr(lr):
    """`WideDeep.check_lr` of the reference: nothing -> the default pair, else a dict with both parts."""
    if not lr:
        return dict(DEFAULT_LR)
    assert isinstance(lr, dict) and "wide" in lr and "deep" in lr, (
        "`lr` should be a dict that contains learning rate of wide and deep parts, e.g. {'wide': 0.01, 'deep': 1e-4}")
    return lr


class WideDeep(_FMCommon):
    def __init__(self, task, data_info=None, loss_type="cross_entropy", embed_size=16, n_epochs=20, lr=None, lr_decay=False,
                 epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, use_bn=True, dropout_rate=None,
                 hidden_units=(128, 64, 32), multi_sparse_combiner="sqrtn", seed=42, lower_upper_bound=None,
                 tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, lower_upper_bound)
        self.all_args = locals()
        self._common(data_info, loss_type, embed_size, n_epochs, check_lr(lr), lr_decay, epsilon, reg, batch_size, sampler,
                     num_neg, use_bn, dropout_rate, multi_sparse_combiner, seed, device, dense_adam)
        self.hidden_units = hidden_units_config(hidden_units)

    def build_model(self):
        self.device = hip_device(self._device_arg)
        self.net = WideDeepNet(self._spec(), self.embed_size, self.hidden_units, self.use_bn, self.dropout_rate, self.lr,
                               self.epsilon, self.seed, self.device, self.dense_adam, self.reg)

    def _hparams(self):
        out = super()._hparams()          # keeps scalars and sequences: the pair of learning rates is a dict
        out["lr"] = {k: float(v) for k, v in self.lr.items()}
        return out

    def current_lr(self):
        """Both learning rates under the staircase of `Base.current_lr` (`tf_trainer.py:283-290`)."""
        net = getattr(self, "net", None)
        if not self.lr_decay or net is None:
            return dict(self.lr)
        decay_steps = max(1, int(self.data_info.data_size / self.batch_size))
        factor = 0.96 ** (int(net.step) // decay_steps)
        return {k: v * factor for k, v in self.lr.items()}

    def apply_lr_schedule(self):
        if self.lr_decay:
            self.net.lr = self.current_lr()

    def save_tf_variables(self, path, model_name):
        raise NotImplementedError("WideDeep: the reference's `*_wide_var` / `*_deep_var` variable names are not mapped")

    def load_tf_variables(self, path, model_name):
        raise NotImplementedError("WideDeep: the reference's `*_wide_var` / `*_deep_var` variable names are not mapped")
