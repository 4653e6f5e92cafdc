"""One NAF network update restated on the host: the oracle's torso layers and TF1 Adam (oracle/nn.py, oracle/optim.py,
unchanged) composed with the head of tests/naf_ref.py — what nn.networks.NAFNet.learn_from_batch computes on the
device.  Also the fixed-batch learning problem that tests/test_naf_ref.py (restatement alone) and tests/test_naf.py
(device against restatement) share."""
import numpy as np

import naf_ref as R
from oracle import nn as N
from oracle.optim import mix_weights

F32 = np.float32
HEAD = "main/naf_q_values_head"


class ComposedNAF(object):
    def __init__(self, arrays, output_scale, activation="relu", head_activation="tanh", lr=1e-3, beta1=0.9, beta2=0.99,
                 eps=1e-4, huber=False, clip_value=None):
        """arrays: {parameter name: [array per tower]} as FlatParams.named_arrays() gives them."""
        self.scale, self.huber, self.clip_value = np.asarray(output_scale, F32), huber, clip_value
        self.nets = []
        for _ in range(2):                                  # online, target
            a = {k: [x.copy() for x in v] for k, v in arrays.items()}
            dense = lambda n, act=None: N.Dense(a[HEAD + "/" + n + "/kernel"][0], a[HEAD + "/" + n + "/bias"][0], act)
            self.nets.append(dict(torso=N.build_chain(a, "main", 0, (1,), activation), V=dense("V"),
                                  mu=dense("mu_unscaled", head_activation), l=dense("l_vector")))
        self.adam = N.PerTensorAdam(lr, beta1, beta2, eps)
        self._torso_names = self._names_of_torso(arrays)

    def named_layers(self, which=0):
        """[(parameter name prefix, layer)] in the device network's naming."""
        net = self.nets[which]
        out = list(zip(self._torso_names, net["torso"].layers))
        return out + [(HEAD + "/V", net["V"]), (HEAD + "/mu_unscaled", net["mu"]), (HEAD + "/l_vector", net["l"])]

    @staticmethod
    def _names_of_torso(arrays):
        names = []
        for part in ("embedder", "middleware"):
            i = 0
            while "main/%s/dense%d/kernel" % (part, i) in arrays:
                names.append("main/%s/dense%d" % (part, i))
                i += 1
        return names

    def weights(self):
        return {n + s: getattr(l, a) for n, l in self.named_layers() for s, a in (("/kernel", "W"), ("/bias", "b"))}

    def update_target(self, rate):
        for (_, lo), (_, lt) in zip(self.named_layers(0), self.named_layers(1)):
            lt.W[...] = mix_weights(lt.W, lo.W, F32(rate))
            lt.b[...] = mix_weights(lt.b, lo.b, F32(rate))

    def learn(self, obs, next_obs, actions, rewards, game_overs, discount):
        on, tg = self.nets
        v_next = tg["V"].forward(tg["torso"].forward(N.prep_obs(next_obs, False)))[:, 0]
        feat = on["torso"].forward(N.prep_obs(obs, False))
        v, mu, l = on["V"].forward(feat), on["mu"].forward(feat), on["l"].forward(feat)
        u = R.update(v[:, 0], mu, l, self.scale, actions, v_next, rewards, game_overs, discount, self.huber)
        self.last = u
        dfeat = on["V"].backward(u["dv"][:, None])
        dfeat = (dfeat + on["mu"].backward(u["dmu_unscaled"])).astype(F32)
        dfeat = (dfeat + on["l"].backward(u["dl"])).astype(F32)
        on["torso"].backward(dfeat)
        for name, layer in self.named_layers():
            if self.clip_value:
                c = F32(self.clip_value)
                layer.dW, layer.db = np.clip(layer.dW, -c, c).astype(F32), np.clip(layer.db, -c, c).astype(F32)
            self.adam.step((name, "k"), layer.W, layer.dW)
            self.adam.step((name, "b"), layer.b, layer.db)
        return float(u["loss"])


def xavier_arrays(obs_dim, A, embedder, middleware, seed):
    """glorot-uniform kernels and zero biases of a NAF network, in FlatParams.named_arrays()'s form."""
    rng = np.random.RandomState(seed)
    arrays, feat = {}, obs_dim

    def dense(name, k, n):
        lim = np.sqrt(6.0 / (k + n))
        arrays[name + "/kernel"] = [rng.uniform(-lim, lim, size=(k, n)).astype(F32)]
        arrays[name + "/bias"] = [np.zeros(n, F32)]
    for part, sizes in (("embedder", embedder), ("middleware", middleware)):
        for i, u in enumerate(sizes):
            dense("main/%s/dense%d" % (part, i), feat, u)
            feat = u
    dense(HEAD + "/V", feat, 1)
    dense(HEAD + "/mu_unscaled", feat, A)
    dense(HEAD + "/l_vector", feat, R.packed_size(A))
    return arrays


FIXED = dict(obs_dim=8, A=3, B=64, embedder=[64], middleware=[64], seed=11, lr=1e-3)


def fixed_batch_problem():
    """rewards = -||u - W s||^2 on one batch of 64 terminal rows: Q can represent it exactly (mu = W s, L = sqrt(2) I,
    V = 0).  -> (obs, actions, rewards, initial arrays, output_scale)."""
    f = FIXED
    rng = np.random.RandomState(f["seed"])
    obs = rng.randn(f["B"], f["obs_dim"]).astype(F32)
    W = (rng.randn(f["obs_dim"], f["A"]) * 0.15).astype(F32)
    actions = rng.uniform(-1, 1, size=(f["B"], f["A"])).astype(F32)
    d = actions.astype(np.float64) - obs.astype(np.float64) @ W.astype(np.float64)
    rewards = (-(d * d).sum(1)).astype(F32)
    arrays = xavier_arrays(f["obs_dim"], f["A"], f["embedder"], f["middleware"], f["seed"] + 1)
    return obs, actions, rewards, arrays, np.ones(f["A"], F32)
