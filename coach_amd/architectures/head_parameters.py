"""Head parameter objects of the network wrappers this engine implements — the subset of
rl_coach/architectures/head_parameters.py the hot-path presets put into
``network_wrappers[...].heads_parameters`` (QHeadParameters :120-130, DuelingQHeadParameters
:132-139).  Only the fields the device networks read are kept."""


class HeadParameters(object):
    head_type = None
    # copies of this head on the same middleware output, each with its own weights (head_parameters.py:22-34); a class
    # default, so that only a network that sets it (Bootstrapped DQN: 10) carries the field
    num_output_head_copies = 1

    def __init__(self, activation_function='relu', name='head', rescale_gradient_from_head_by_factor=1.0,
                 loss_weight=1.0):
        self.activation_function = activation_function
        self.name = name
        # the gradient entering the middleware from this head is multiplied by this factor
        # (general_network.py:296-303: head_input = (1 - f) * stop_gradient(x) + f * x)
        self.rescale_gradient_from_head_by_factor = rescale_gradient_from_head_by_factor
        self.loss_weight = loss_weight


class QHeadParameters(HeadParameters):
    head_type = "QHead"

    def __init__(self, activation_function='relu', name='q_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class DuelingQHeadParameters(HeadParameters):
    head_type = "DuelingQHead"

    def __init__(self, activation_function='relu', name='dueling_q_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class ClassificationHeadParameters(HeadParameters):
    """head_parameters.py:194-201 — Dense(A) class logits under a softmax, the softmax cross entropy summed over the batch
    (heads/classification_head.py).  Served by nn.networks.ClassificationNet (rlx_classification_head_loss) and
    ClassificationArchitecture: Batch RL's imitation model (agents/ddqn_bcq_agent.py, NNImitationModelParameters)."""
    head_type = "ClassificationHead"

    def __init__(self, activation_function='relu', name='classification_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class QuantileRegressionQHeadParameters(HeadParameters):
    """QuantileRegressionQHeadParameters (head_parameters.py:204-212): one Dense layer of A * atoms outputs, read as
    [batch, A, atoms] (heads/quantile_regression_q_head.py:40-81); the atom count is the algorithm's `atoms`."""
    head_type = "QuantileRegressionQHead"

    def __init__(self, activation_function='relu', name='quantile_regression_q_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class CategoricalQHeadParameters(HeadParameters):
    """CategoricalQHeadParameters (head_parameters.py:76-85): one Dense layer of A * atoms logits, read as
    [batch, A, atoms] with a softmax over the atoms (heads/categorical_q_head.py:42-58); the support is the algorithm's
    np.linspace(v_min, v_max, atoms)."""
    head_type = "CategoricalQHead"

    def __init__(self, activation_function='relu', name='categorical_q_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class RainbowQHeadParameters(HeadParameters):
    """RainbowQHeadParameters (head_parameters.py:215-222): a dueling head over atoms — a state-value stream
    Dense(512, activation) -> Dense(atoms) and an action-advantage stream Dense(512, activation) -> Dense(A * atoms),
    merged per atom, with a softmax over the atoms (heads/rainbow_q_head.py:38-70).  The merge, the projection, the cross
    entropy and the gradients of the two stream outputs come from rlx_rainbow_head_loss."""
    head_type = "RainbowQHead"

    def __init__(self, activation_function='relu', name='rainbow_q_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class NAFHeadParameters(HeadParameters):
    """NAFHeadParameters (head_parameters.py:152-159): three Dense layers on the middleware's output — V (1),
    mu_unscaled (A, this activation, then times the action space's max_abs_range) and l_vector (A(A+1)/2), read as a
    lower-triangular matrix with an exponentiated diagonal (heads/naf_head.py:45-86)."""
    head_type = "NAFHead"

    def __init__(self, activation_function='tanh', name='naf_head_params', rescale_gradient_from_head_by_factor=1.0,
                 loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class WolpertingerActorHeadParameters(HeadParameters):
    """WolpertingerActorHeadParameters (head_parameters.py:111-119): one Dense layer of action_embedding_width outputs
    ('actor_action_embedding'), optional batch normalisation, this activation, then times the filtered box space's
    max_abs_range (heads/wolpertinger_actor_head.py:43-56) — the DDPG actor head with the embedding width for its
    action count, which is what ActorNet builds.  The class default of `batchnorm` is the reference's (True); the agent's
    network parameters pass use_batchnorm."""
    head_type = "WolpertingerActorHead"

    def __init__(self, activation_function='tanh', name='policy_head_params', batchnorm=True,
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)
        self.batchnorm = batchnorm


class PolicyHeadParameters(HeadParameters):
    """PolicyHeadParameters (head_parameters.py:162-169): for a discrete action space one Dense layer of A policy values
    ('fc') under a softmax (heads/policy_head.py:89-100; the activation is the continuous branch's, which has no device
    form).  The loss -mean(log pi(a) * advantage) and the entropy regularisation come from rlx_pg_head_loss."""
    head_type = "PolicyHead"

    def __init__(self, activation_function='tanh', name='policy_head_params', rescale_gradient_from_head_by_factor=1.0,
                 loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class VHeadParameters(HeadParameters):
    """VHeadParameters (head_parameters.py:50-60): one Dense layer of one output on the middleware's output, normalized-
    columns initialisation with std 1.0 (heads/v_head.py:43-48), MSE against the value targets under `loss_weight`.
    Actor-Critic's loss and gradient come from rlx_a3c_window_loss."""
    head_type = "VHead"

    def __init__(self, activation_function='relu', name='v_head_params', rescale_gradient_from_head_by_factor=1.0,
                 loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class ACERPolicyHeadParameters(HeadParameters):
    """ACERPolicyHeadParameters (head_parameters.py:225-232): for a discrete action space one Dense layer of A policy
    values ('fc') under a softmax (heads/acer_policy_head.py:115-125).  The truncated importance-weighted loss, the bias
    correction, the KL to the average policy and the optional trust-region step come from rlx_acer_window_loss."""
    head_type = "ACERPolicyHead"

    def __init__(self, activation_function='relu', name='acer_policy_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)


class MeasurementsPredictionHeadParameters(HeadParameters):
    """MeasurementsPredictionHeadParameters (head_parameters.py:141-149): an expectation stream Dense(256, activation) ->
    Dense(K) and an action stream Dense(256, activation) -> Dense(A * K), K = num_predicted_steps_ahead * measurements,
    merged like a dueling head (heads/measurements_prediction_head.py:39-57).  The merge, the NaN-ignoring squared loss
    and the gradients of the two stream outputs come from rlx_dfp_head_loss."""
    head_type = "MeasurementsPredictionHead"

    def __init__(self, activation_function='relu', name='measurements_prediction_head_params',
                 rescale_gradient_from_head_by_factor=1.0, loss_weight=1.0):
        super().__init__(activation_function, name, rescale_gradient_from_head_by_factor, loss_weight)
