"""sgdnet_amd: MI355X (gfx950) SAGA elastic-net backend behind the sgdnet() API.

The compute lives in sgdnet_amd/lib/libsgdnet_hip.so (hand-written HIP, C ABI in
include/sgdnet_hip.h).  This package is the host-side mirror of the reference's
R front-end for the fit path plus benchmark/multi-GPU plumbing.
"""
from ._lib import LIB_PATH, SgdnetError, load  # noqa: F401
from .api import SgdnetFit, sgdnet, sgdnet_mcovariance, sgdnet_mnewton, sgdnet_newton, sgdnet_wcovariance, sgdnet_wmcovariance, sgdnet_wmnewton, sgdnet_wnewton  # noqa: F401
from .cv import (CvSgdnet, cv_covariance_fits, cv_mcovariance_fits, cv_mnewton_fits, cv_newton_fits, cv_sgdnet,  # noqa: F401
                 cv_sgdnet_mcovariance, cv_sgdnet_mnewton, cv_sgdnet_newton, cv_sgdnet_wcovariance, cv_sgdnet_wmcovariance, cv_wcovariance_fits,
                 cv_wmcovariance_fits, cv_sgdnet_wnewton, cv_wnewton_fits)
from .kkt import (evaluation_intercepts, feature_moments, kkt, kkt_from_gradient, path_gradient,  # noqa: F401
                  response_moments)
from .predict import coef, predict  # noqa: F401
from .score import score  # noqa: F401
from .solver import (RRng, SagaSolver, auto_batch, covariance_max_features, get_option, link_peers, mcovariance_max_features, mnewton_max_features, newton_max_features, option, set_option, wcovariance_max_features, wmcovariance_max_features, wmnewton_max_features, wnewton_max_features,  # noqa: F401
                     shard_window)

__all__ = ["sgdnet", "SgdnetFit", "SagaSolver", "RRng", "auto_batch", "SgdnetError", "load", "LIB_PATH",
           "cv_sgdnet", "CvSgdnet", "predict", "coef", "score", "set_option", "get_option", "option",
           "path_gradient", "kkt_from_gradient", "kkt", "feature_moments", "response_moments", "evaluation_intercepts",
           "covariance_max_features", "cv_covariance_fits", "sgdnet_newton", "newton_max_features",
           "cv_newton_fits", "cv_sgdnet_newton", "sgdnet_mcovariance", "mcovariance_max_features",
           "sgdnet_mnewton", "mnewton_max_features", "sgdnet_wcovariance", "wcovariance_max_features",
           "sgdnet_wnewton", "wnewton_max_features", "sgdnet_wmcovariance", "wmcovariance_max_features",
           "sgdnet_wmnewton", "wmnewton_max_features", "cv_mcovariance_fits", "cv_sgdnet_mcovariance",
           "cv_mnewton_fits", "cv_sgdnet_mnewton", "cv_wcovariance_fits", "cv_sgdnet_wcovariance",
           "cv_wmcovariance_fits", "cv_sgdnet_wmcovariance", "cv_wnewton_fits", "cv_sgdnet_wnewton"]
