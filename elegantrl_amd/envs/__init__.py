from .vec_envs import CartPoleGpuVecEnv, CartPoleVecEnv, PendulumVecEnv, SynVecEnv
