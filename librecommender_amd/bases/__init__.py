from .base import Base
from .cf_base import CfBase
from .cf_base_rs import RsCfBase
from .embed_base import EmbedBase
from .dyn_embed_base import DynEmbedBase
from .feat_base import FeatBase
from .word2vec_base import Word2VecBase
from .sage_base import SageBase

GensimBase = Word2VecBase      # the reference's name for this base

__all__ = ["Base", "CfBase", "RsCfBase", "EmbedBase", "DynEmbedBase", "FeatBase", "Word2VecBase", "GensimBase", "SageBase"]
