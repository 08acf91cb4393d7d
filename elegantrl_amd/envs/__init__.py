from .vec_envs import (AcrobotGpuVecEnv, CartPoleGpuVecEnv, CartPoleVecEnv, MountainCarGpuVecEnv, PendulumVecEnv, PointChasingVecEnv,
                       SynVecEnv)
