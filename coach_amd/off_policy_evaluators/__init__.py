"""Off-policy evaluators of Batch RL (rl_coach/off_policy_evaluators): see ope_manager.py."""
