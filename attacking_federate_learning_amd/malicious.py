"""Drop-in replacement for the reference's `malicious` module (reference malicious.py:1-36).

`Attack.attack(users)` keeps the reference's contract: it reads `usr.grads` of every malicious user, stores
`grads_mean` / `grads_stdev` on the attacker, returns early when `num_std == 0`, otherwise calls the
overridable hook `_attack_grads(grads_mean, grads_stdev, original_params, learning_rate)` with host arrays
and rebinds every `usr.grads` to the ONE array the hook returned (reference malicious.py:26-27).
`backdoor.BackdoorAttack` subclasses `Attack` and overrides only the hook, which keeps working.

Beyond the reference: `FangTrimmedMeanAttack` and `FangKrumAttack`, the adaptive attacks of Fang et al. (USENIX Security 2020)
on the trimmed mean / median and on Krum; they need the benign gradients too and give every malicious user its own row.

`MinMaxAttack` and `MinSumAttack` are the AGR-agnostic attacks of Shejwalkar and Houmansadr (NDSS 2021, section IV-C); like
`DriftAttack` they give every malicious user the ONE shared array.

The column statistics run in libbyzagg's column kernel; for `DriftAttack` the drift itself is fused into
that kernel, so the m x D matrix is read once.
"""
import numpy as np

from .engine import get_engine


class Attack(object):
    def __init__(self, num_std):
        self.num_std = num_std
        self.grads_mean = None
        self.grads_stdev = None

    def _statistics(self, users, num_std):
        rows = np.stack([np.asarray(usr.grads, dtype=np.float32) for usr in users])
        return get_engine().drift_attack(rows, num_std)

    def attack(self, users):
        if len(users) == 0:
            return

        drift, self.grads_mean, self.grads_stdev = self._statistics(users, self.num_std)

        if self.num_std == 0:
            return

        mal_grads = self._attack_grads(self.grads_mean, self.grads_stdev, users[0].original_params,
                                       users[0].learning_rate)

        for usr in users:
            usr.grads = mal_grads


class DriftAttack(Attack):
    def __init__(self, num_std):
        super(DriftAttack, self).__init__(num_std)
        self._fused = None

    def attack(self, users):
        if len(users) == 0:
            return
        # one kernel produces mean, std and mean - z*std; the hook below hands the fused vector back
        self._fused, self.grads_mean, self.grads_stdev = self._statistics(users, self.num_std)
        if self.num_std == 0:
            self._fused = None
            return
        mal_grads = self._attack_grads(self.grads_mean, self.grads_stdev, users[0].original_params,
                                       users[0].learning_rate)
        self._fused = None
        for usr in users:
            usr.grads = mal_grads

    def _attack_grads(self, grads_mean, grads_stdev, original_params, learning_rate):
        """mean[:] -= num_std * std[:], in place, returns `grads_mean` (reference malicious.py:34-36)."""
        if self._fused is not None and grads_mean is self.grads_mean:
            grads_mean[:] = self._fused
        else:  # called directly with arbitrary vectors
            grads_mean[:] = get_engine().drift_axpy_host(grads_mean, grads_stdev, self.num_std)
        return grads_mean


class _FangAttack(Attack):
    """What the two attacks of Fang, Cao, Jia and Gong (USENIX Security 2020) share: they need the BENIGN gradients as well
    (full knowledge), passed as `attack(users, benign_users=...)` or bound beforehand with `bind(matrix)`; `num_std` is not
    read (it is None).  `grads_mean` / `grads_stdev` are kept as `Attack.attack` keeps them."""

    def __init__(self):
        super(_FangAttack, self).__init__(None)
        self.benign = None

    def bind(self, benign):
        """The benign clients' gradients for the calls that follow: a 2-D float32 array, one row a client (None: unbind)."""
        self.benign = None if benign is None else np.ascontiguousarray(benign, dtype=np.float32)
        return self

    def _matrix(self, users, benign_users, needs_benign):
        rows = np.stack([np.asarray(usr.grads, dtype=np.float32) for usr in users])
        if benign_users is not None:
            benign = np.stack([np.asarray(usr.grads, dtype=np.float32) for usr in benign_users])
        else:
            benign = self.benign
        if benign is None:
            if needs_benign:
                raise ValueError('%s needs the benign gradients: attack(users, benign_users=...) or bind(matrix)'
                                 % type(self).__name__)
            return rows
        return np.concatenate([rows, benign.reshape(-1, rows.shape[1])])

    def _hand_out(self, users, attacked):
        for usr, row in zip(users, attacked):
            usr.grads = row


class FangTrimmedMeanAttack(_FangAttack):
    """The trimmed-mean / median attack (section 4.3): per coordinate every malicious value is drawn beyond the benign extreme
    on the side that turns the aggregate round -- from [lo / b, lo] or [b lo, lo] where the column mean is above 0, from
    [hi, b hi] or [hi, hi / b] otherwise.  partial=True is the paper's partial-knowledge variant, from the malicious clients' own
    mean and std alone: [mu - 4 sigma, mu - 3 sigma] or [mu + 3 sigma, mu + 4 sigma]; it needs no benign gradients.
    UNLIKE DriftAttack, which rebinds every malicious `usr.grads` to ONE shared array (reference malicious.py:26-27), every
    malicious user gets ITS OWN row here: the paper samples c numbers per coordinate.  The draws are a function of (seed, the
    number of earlier calls, the user's position, the coordinate): `round` counts the calls."""

    def __init__(self, b=2.0, partial=False, seed=0):
        super(FangTrimmedMeanAttack, self).__init__()
        self.b, self.partial, self.seed, self.round = b, bool(partial), seed, 0

    def attack(self, users, benign_users=None):
        if len(users) == 0:
            return
        _, self.grads_mean, self.grads_stdev = self._statistics(users, 0.0)
        g = self._matrix(users, None if self.partial else benign_users, needs_benign=not self.partial)
        attacked = get_engine().fang_trmean_attack(g, len(users), b=self.b, partial=self.partial, seed=self.seed, round=self.round)
        self.round += 1
        self._hand_out(users, attacked)


class FangKrumAttack(_FangAttack):
    """The Krum attack (section 4.2): every malicious gradient becomes -lambda s, s the sign of the column means, with the
    largest lambda = lambda_0 / 2^k for which Krum over all the clients picks a malicious one (lambda_0: the paper's Theorem 1);
    below `threshold` the search gives up and keeps its last lambda.  The paper's other malicious vectors "within epsilon of
    the first" are copies of it, as in every public implementation; each user still gets its own row.  `info` holds the last
    call's {lambda0, lambda, steps, chosen, succeeded}."""

    def __init__(self, threshold=1e-5):
        super(FangKrumAttack, self).__init__()
        self.threshold, self.info = threshold, None

    def attack(self, users, benign_users=None):
        if len(users) == 0:
            return
        _, self.grads_mean, self.grads_stdev = self._statistics(users, 0.0)
        g = self._matrix(users, benign_users, needs_benign=True)
        attacked, self.info = get_engine().fang_krum_attack(g, len(users), threshold=self.threshold, return_info=True)
        self._hand_out(users, attacked)


class _AgnosticAttack(_FangAttack):
    """What Min-Max and Min-Sum (Shejwalkar and Houmansadr, NDSS 2021, section IV-C) share: every malicious gradient becomes
    the ONE vector mu + gamma p, gamma in closed form (include/byzagg.h, rule D).  perturbation: 'unit', 'std' (the population
    std; the authors' torch.std gives the same vector from a gamma smaller by sqrt((r - 1) / r)) or 'sign'.  partial=True knows
    the malicious clients' gradients alone; otherwise the benign ones come through `attack(users, benign_users=...)` or
    `bind(matrix)`.  Every malicious `usr.grads` is rebound to ONE array, as DriftAttack does; `info` holds the last call's
    report.  A broken call (a value that is not finite) leaves the users' gradients as they were."""

    kind = None

    def __init__(self, perturbation='std', partial=False):
        from .engine import MINMAX_PERTURBATIONS
        if perturbation not in MINMAX_PERTURBATIONS or perturbation == 'custom':
            raise ValueError("perturbation = %r: 'unit', 'std' or 'sign'" % (perturbation,))
        super(_AgnosticAttack, self).__init__()
        self.perturbation, self.partial, self.info = perturbation, bool(partial), None

    def attack(self, users, benign_users=None):
        if len(users) == 0:
            return
        g = self._matrix(users, None if self.partial else benign_users, needs_benign=not self.partial)
        _, self.grads_mean, self.grads_stdev = self._statistics(users, 0.0)
        vector, self.info = get_engine().minmax_attack(g, len(users), kind=self.kind, perturbation=self.perturbation,
                                                       partial=self.partial, return_info=True)
        if self.info['broken']:
            return
        for usr in users:
            usr.grads = vector


class MinMaxAttack(_AgnosticAttack):
    """Min-Max: the malicious vector's largest distance to a known gradient stays within the largest distance between two known
    gradients."""
    kind = 'minmax'


class MinSumAttack(_AgnosticAttack):
    """Min-Sum: the malicious vector's summed squared distance to the known gradients stays within the largest such sum of a
    known gradient.  No distance matrix: two reads of the gradients."""
    kind = 'minsum'
