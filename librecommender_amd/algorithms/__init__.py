from .als import ALS
from .autoint import AutoInt
from .bpr import BPR
from .caser import Caser
from .deepwalk import DeepWalk
from .din import DIN
from .fm import FM, DeepFM
from .graphsage import GraphSage
from .item2vec import Item2Vec
from .item_cf import ItemCF
from .item_cf_rs import RsItemCF
from .lightgcn import LightGCN
from .ncf import NCF
from .ngcf import NGCF
from .pinsage import PinSage
from .rnn4rec import RNN4Rec
from .sim import SIM
from .svd import SVD
from .svdpp import SVDpp
from .swing import Swing
from .transformer import Transformer
from .two_tower import TwoTower
from .user_cf import UserCF
from .user_cf_rs import RsUserCF
from .wavenet import WaveNet
from .wide_deep import WideDeep
from .youtube_ranking import YouTubeRanking
from .youtube_retrieval import YouTubeRetrieval

__all__ = ["ALS", "AutoInt", "BPR", "Caser", "DIN", "DeepFM", "DeepWalk", "FM", "GraphSage", "Item2Vec", "ItemCF", "LightGCN", "NCF", "NGCF", "PinSage", "RNN4Rec", "RsItemCF", "RsUserCF", "SIM", "SVD", "SVDpp", "Swing", "Transformer", "TwoTower", "UserCF", "WaveNet", "WideDeep", "YouTubeRanking", "YouTubeRetrieval"]
