"""Learning-loop surfaces (reference src/learning): novelty-based data selection."""
from .novelty_selector import ActiveDataSelector, DataBuffer, NoveltyConfig, NoveltySelector

__all__ = ["ActiveDataSelector", "DataBuffer", "NoveltyConfig", "NoveltySelector"]
