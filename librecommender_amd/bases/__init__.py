from .base import Base
from .cf_base import CfBase
from .embed_base import EmbedBase
from .feat_base import FeatBase

__all__ = ["Base", "CfBase", "EmbedBase", "FeatBase"]
