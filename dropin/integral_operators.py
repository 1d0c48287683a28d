"""``from integral_operators import *`` -> the MI355X-native operator blocks (the same alias as the repository root's)."""
from uno_amd.integral_operators import *  # noqa: F401,F403
from uno_amd.integral_operators import __all__  # noqa: F401
