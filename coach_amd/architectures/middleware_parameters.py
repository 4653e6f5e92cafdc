"""`FCMiddlewareParameters(...)` / `LSTMMiddlewareParameters(...)` — the records reference presets assign to
`network_wrappers[...].middleware_parameters` (rl_coach/architectures/middleware_parameters.py:22-59), with the
reference's signatures.  The device network parameter classes keep flat fields; `SchemeViews.middleware_parameters`'
setter folds a record into them (coach_amd/architectures/scheme_views.py): the scheme, and for the LSTM record the flat
`lstm_cells` the recurrent Actor-Critic networks are built from (nn/networks.py, csrc/lstm.hip)."""
from ..base_parameters import MiddlewareScheme


class MiddlewareParameters(object):
    def __init__(self, parameterized_class_name, activation_function='relu', scheme=MiddlewareScheme.Medium,
                 batchnorm=False, dropout_rate=0.0, name='middleware', dense_layer=None, is_training=False):
        self.parameterized_class_name = parameterized_class_name
        self.activation_function = activation_function
        self.scheme = scheme
        self.batchnorm = batchnorm
        self.dropout_rate = dropout_rate
        self.name = name
        self.dense_layer = dense_layer
        self.is_training = is_training


class FCMiddlewareParameters(MiddlewareParameters):
    def __init__(self, activation_function='relu', scheme=MiddlewareScheme.Medium, batchnorm=False, dropout_rate=0.0,
                 name="middleware_fc_embedder", dense_layer=None, is_training=False, num_streams=1):
        super().__init__("FCMiddleware", activation_function, scheme, batchnorm, dropout_rate, name, dense_layer,
                         is_training)
        self.num_streams = num_streams


class LSTMMiddlewareParameters(MiddlewareParameters):
    def __init__(self, activation_function='relu', number_of_lstm_cells=256, scheme=MiddlewareScheme.Medium,
                 batchnorm=False, dropout_rate=0.0, name="middleware_lstm_embedder", dense_layer=None, is_training=False):
        super().__init__("LSTMMiddleware", activation_function, scheme, batchnorm, dropout_rate, name, dense_layer,
                         is_training)
        self.number_of_lstm_cells = number_of_lstm_cells


def refuse_lstm_middleware(agent_parameters, who):
    """every agent but Actor-Critic: an LSTM middleware on any of its networks is refused by name"""
    for name, w in getattr(agent_parameters, "network_wrappers", {}).items():
        if getattr(w, "lstm_cells", None) is not None or \
                isinstance(w.__dict__.get("middleware_parameters"), LSTMMiddlewareParameters):
            raise ValueError("LSTMMiddlewareParameters on network %r: the LSTM middleware is served under the "
                             "Actor-Critic agent only, not under %s" % (name, who))
