from ._neighbors import neighbors

__all__ = ["neighbors"]
