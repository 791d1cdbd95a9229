"""Device-side computation graphs of the north-star models (what `build_model()` creates in the
reference), expressed over the HIP hot-path kernels + torch dense layers."""
from .autoint_net import FeatAutoIntNet
from .caser_net import CaserNet
from .feat_embedding import FeatEmbedding, FeatSpec
from .feat_nets import FeatDeepFMNet, FeatDINNet, FeatFMNet, FeatYouTubeRankingNet, ShardedDINNet
from .field_parallel import FieldParallelDeepFMNet
from .fm_nets import DeepFMNet, FMNet, ShardedDeepFMNet, ShardedFMNet
from .ncf_net import NCFNet
from .ngcf_net import NGCFNet
from .rnn_nets import RNN4RecNet
from .sage_net import SageNet
from .pinsage_net import PinSageNet
from .wavenet_net import WaveNetNet
from .wide_deep_net import WideDeepNet
from .tower_nets import ShardedTwoTowerNet, TwoTowerNet

__all__ = ["DeepFMNet", "FMNet", "ShardedDeepFMNet", "ShardedFMNet", "FieldParallelDeepFMNet", "TwoTowerNet", "ShardedTwoTowerNet", "FeatEmbedding",
           "FeatSpec", "FeatDeepFMNet", "FeatDINNet", "FeatFMNet", "FeatYouTubeRankingNet", "ShardedDINNet", "NGCFNet", "RNN4RecNet", "WaveNetNet", "FeatAutoIntNet", "CaserNet", "SageNet", "PinSageNet", "WideDeepNet", "NCFNet"]
