"""sfm_amd: MI355X-native matching + bundle-adjustment hot path."""

from .twoview import FundamentalMixin, estimate_fundamental_batched, find_fundamental  # noqa: F401
