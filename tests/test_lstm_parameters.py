"""Host side of the LSTM middleware: the reference preset's text through coach_amd.compat, and the refusals by name."""
import pytest

from test_preset_dropin import _exec_preset, _text, needs_reference


@needs_reference
def test_reference_mujoco_a3c_lstm_preset_text_reaches_the_flat_fields():
    w = _exec_preset(_text("Mujoco_A3C_LSTM"))["agent_params"].network_wrappers["main"]
    assert (w.embedder_scheme, w.middleware_scheme, w.lstm_cells, w.learning_rate) == ([200], "Empty", 128, 0.00002)


def test_refusals_name_what_they_refuse():
    from coach_amd.agents.actor_critic_agent import ActorCriticAgentParameters
    from coach_amd.agents.dqn_agent import DQNAgent, DQNAgentParameters
    from coach_amd.architectures.hip_architecture import ActorCriticArchitecture
    from coach_amd.architectures.middleware_parameters import FCMiddlewareParameters, LSTMMiddlewareParameters
    w = ActorCriticAgentParameters().network_wrappers["main"]
    for kw, named in ((dict(batchnorm=True), "batchnorm"), (dict(dropout_rate=0.3), "dropout_rate")):
        with pytest.raises(ValueError, match=named):
            w.middleware_parameters = LSTMMiddlewareParameters(**kw)
    w.middleware_parameters = LSTMMiddlewareParameters(number_of_lstm_cells=32)
    assert (w.middleware_scheme, w.lstm_cells) == ("Medium", 32)
    with pytest.raises(ValueError, match="LSTMMiddlewareParameters"):
        ActorCriticArchitecture._build(None, None, None, w, 0)
    w.middleware_parameters = FCMiddlewareParameters(scheme="Shallow")
    assert (w.middleware_scheme, w.lstm_cells) == ("Shallow", None)
    dqn = DQNAgentParameters()
    with pytest.raises(ValueError, match="LSTMMiddlewareParameters"):
        dqn.network_wrappers["main"].middleware_parameters = LSTMMiddlewareParameters()
    dqn.network_wrappers["main"].lstm_cells = 32                      # past the setter: the agent refuses too
    with pytest.raises(ValueError, match="LSTMMiddlewareParameters.*DQNAgent"):
        DQNAgent(dqn, None)
