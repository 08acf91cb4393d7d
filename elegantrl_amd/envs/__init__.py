from .vec_envs import AcrobotGpuVecEnv, CartPoleGpuVecEnv, CartPoleVecEnv, PendulumVecEnv, SynVecEnv
