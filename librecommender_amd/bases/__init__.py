from .base import Base
from .cf_base import CfBase
from .embed_base import EmbedBase
from .dyn_embed_base import DynEmbedBase
from .feat_base import FeatBase

__all__ = ["Base", "CfBase", "EmbedBase", "DynEmbedBase", "FeatBase"]
