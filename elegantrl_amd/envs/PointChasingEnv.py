"""`from elegantrl.envs.PointChasingEnv import PointChasingVecEnv` (the reference's import path) resolves here through `compat`."""
from .vec_envs import PointChasingVecEnv  # noqa: F401
