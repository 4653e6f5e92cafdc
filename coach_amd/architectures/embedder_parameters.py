"""`InputEmbedderParameters(scheme=...)` — the record reference presets put into
`network_wrappers[...].input_embedders_parameters` (rl_coach/architectures/embedder_parameters.py:25-45).  The device
network parameter classes keep flat fields; `SchemeViews.input_embedders_parameters`' setter folds these records into
them (coach_amd/architectures/scheme_views.py)."""
from ..base_parameters import EmbedderScheme, MiddlewareScheme  # noqa: F401  (presets import both from here too)


class InputEmbedderParameters(object):
    def __init__(self, activation_function='relu', scheme=EmbedderScheme.Medium, batchnorm=False, dropout_rate=0.0,
                 name='embedder', input_rescaling=None, input_offset=None, input_clipping=None, dense_layer=None,
                 is_training=False, flatten=True):
        self.activation_function = activation_function
        self.scheme = scheme
        self.batchnorm = batchnorm
        self.dropout_rate = dropout_rate
        self.name = name
        self.input_rescaling = input_rescaling if input_rescaling is not None else \
            {'image': 255.0, 'vector': 1.0, 'tensor': 1.0}
        self.input_offset = input_offset if input_offset is not None else {'image': 0.0, 'vector': 0.0, 'tensor': 0.0}
        self.input_clipping = input_clipping
        self.dense_layer = dense_layer
        self.is_training = is_training
        self.flatten = flatten
