"""`import malicious` shim: see dropin/defences.py."""
from attacking_federate_learning_amd.malicious import Attack, DriftAttack, FangKrumAttack, FangTrimmedMeanAttack, MinMaxAttack, MinSumAttack  # noqa: F401
