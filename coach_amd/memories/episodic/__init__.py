"""rl_coach/memories/episodic/__init__.py exports its memories' parameter classes; presets import them from here."""
from .episodic_experience_replay import EpisodicExperienceReplayParameters
from .episodic_hindsight_experience_replay import EpisodicHindsightExperienceReplayParameters
from .single_episode_buffer import SingleEpisodeBufferParameters

__all__ = ['EpisodicExperienceReplayParameters', 'EpisodicHindsightExperienceReplayParameters',
           'SingleEpisodeBufferParameters']
