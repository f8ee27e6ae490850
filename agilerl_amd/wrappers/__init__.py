from .learning import BanditEnv

__all__ = ["BanditEnv"]
