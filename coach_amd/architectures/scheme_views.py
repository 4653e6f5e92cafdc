"""`network_wrappers[...].input_embedders_parameters['observation'].scheme = [Dense(400)]`,
`.middleware_parameters.scheme = ...`, `.heads_parameters[0].network_layers_sizes = ...` — the way reference
presets reach into NetworkParameters (base_parameters.py:226-305, embedder_parameters.py, middleware_parameters.py).
The device network parameter classes keep flat fields (`embedder_scheme`, `middleware_scheme`, ...); this mixin
gives them the reference's nested access path as live views onto those fields."""
from .layers import scheme_to_native


class _SchemeView(object):
    def __init__(self, owner, field, as_tuple):
        object.__setattr__(self, "_owner", owner)
        object.__setattr__(self, "_field", field)
        object.__setattr__(self, "_as_tuple", as_tuple)
        object.__setattr__(self, "_extra", owner.__dict__.setdefault("_view_extras", {}).setdefault(field, {}))

    @property
    def scheme(self):
        return getattr(self._owner, self._field)

    @scheme.setter
    def scheme(self, value):
        setattr(self._owner, self._field, scheme_to_native(value, self._as_tuple))

    @property
    def activation_function(self):
        return self._owner.activation_function

    @activation_function.setter
    def activation_function(self, value):
        self._owner.activation_function = value

    def __getattr__(self, name):                      # dropout_rate, ...: remembered, not used
        extra = object.__getattribute__(self, "_extra")
        if name in extra:
            return extra[name]
        owner = object.__getattribute__(self, "_owner")
        if name == "batchnorm" and hasattr(owner, "batchnorm"):
            return owner.batchnorm
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in ("scheme", "activation_function"):
            object.__setattr__(self, name, value)
        else:
            self._extra[name] = value
            if name == "batchnorm" and hasattr(self._owner, "batchnorm"):
                # the device DDPG networks switch batch normalisation on for the whole network (what
                # DDPGAgentParameters(use_batchnorm=True) does, ddpg_agent.py:37-60), not per component
                self._owner.batchnorm = bool(value)


class SchemeViews(object):
    """Mix into a network-parameters class.  _EMBEDDER_FIELDS: {'observation': field[, 'action': field]};
    _TUPLE_SCHEMES: the fields hold tuples of unit counts (actor-critic nets) instead of names / lists."""
    _EMBEDDER_FIELDS = {"observation": "embedder_scheme"}
    _MIDDLEWARE_FIELD = "middleware_scheme"
    _TUPLE_SCHEMES = False

    @property
    def input_embedders_parameters(self):
        names = self.__dict__.get("input_embedder_names")
        if names is not None:            # several Empty vector embedders over one concatenated observation (see the setter)
            field = self._EMBEDDER_FIELDS["observation"]
            return {k: _SchemeView(self, field, self._TUPLE_SCHEMES) for k in names}
        return {k: _SchemeView(self, f, self._TUPLE_SCHEMES) for k, f in self._EMBEDDER_FIELDS.items()
                if hasattr(self, f)}

    @input_embedders_parameters.setter
    def input_embedders_parameters(self, value):
        """`input_embedders_parameters = {...}` of a preset text.  Accepted: (a) the class's own entries ('observation'
        [, 'action']) — each record's `scheme` goes to its flat field; (b) several named vector embedders that are ALL
        `Empty`: the reference concatenates its embedders' outputs in sorted() name order (general_network.py:252,277),
        so with nothing but Empty embedders the middleware sees the concatenation of the named observations — which is
        the ONE observation vector an environment with a slice table emits.  The names are kept in
        `input_embedder_names` (sorted) and checked against the environment's slices when the agent is built.
        Anything else has no device network and raises."""
        if not isinstance(value, dict) or not value:
            raise ValueError("input_embedders_parameters takes a non-empty dict of embedder parameter records")
        fields = {k: f for k, f in self._EMBEDDER_FIELDS.items() if hasattr(self, f)}
        if set(value) == set(fields):
            for k, rec in value.items():
                setattr(self, fields[k], scheme_to_native(rec.scheme, self._TUPLE_SCHEMES))
            self.__dict__.pop("input_embedder_names", None)
            return
        empty = all(getattr(getattr(rec, "scheme", None), "name", getattr(rec, "scheme", None)) == "Empty"
                    for rec in value.values())
        if list(fields) != ["observation"] or len(value) < 2 or not empty:
            raise ValueError("supported input embedders: {} or several named vector embedders whose scheme is Empty "
                             "(got {})".format(sorted(fields), {k: getattr(v, "scheme", v) for k, v in value.items()}))
        setattr(self, fields["observation"], scheme_to_native(next(iter(value.values())).scheme, self._TUPLE_SCHEMES))
        self.__dict__["input_embedder_names"] = tuple(sorted(value))

    @property
    def middleware_parameters(self):
        return _SchemeView(self, self._MIDDLEWARE_FIELD, self._TUPLE_SCHEMES)
