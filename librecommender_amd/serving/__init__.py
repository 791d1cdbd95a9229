from .embed_server import EmbedServer, InvalidUser
from .export import save_embed, save_ivf_index, save_ivf_sq8_index, save_knn, save_online

__all__ = ["EmbedServer", "InvalidUser", "save_embed", "save_ivf_index", "save_ivf_sq8_index", "save_knn", "save_online"]
