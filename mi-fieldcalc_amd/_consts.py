"""The constants of the Python front: a leaf module, so that the method families can share them without importing the
package back."""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2  # miutil::ValuesDefined, FieldDefined.h:41
UNDEF = np.float32(1.0e35)  # miutil::UNDEF, FieldDefined.cc:34
MEM_HOST, MEM_DEVICE = 0, 1

# mifc_ens_product.stat (include/mifc.h), and the names Context.ensembleStatistics takes for them
ENS_SUM, ENS_MEAN, ENS_STDDEV, ENS_EXTREME, ENS_PROBABILITY = 0, 1, 2, 3, 4
# the product codes of mifc_vlayer_* (include/mifc.h, MIFC_VLAYER_*) and the names Context.vlayer_* takes for them
VLAYER_PRODUCTS = {"integral": 1, "mean": 2, "max": 3, "min": 4, "coord_of_max": 5, "coord_of_min": 6}
# the methods of mifc_vderiv_* (MIFC_VDERIV_*)
VDERIV_METHODS = {"centred": 0, "weighted": 1}
# the methods and walk directions of mifc_vcumul_* (MIFC_VCUMUL_*)
VCUMUL_METHODS = {"linear": 0, "log": 1}
VCUMUL_FROM = {"first": 0, "last": 1}
# the search directions and the treatment of targets outside the column of mifc_vregrid_* (MIFC_VREGRID_*)
VREGRID_METHODS = {"linear": 0, "log": 1}  # MIFC_VINTERP_LINEAR / _LOG
VREGRID_FROM = {"first": 0, "last": 1}
VREGRID_OUTSIDE = {"undef": 0, "clamp": 1}
# the walk directions of mifc_vparcel_* (MIFC_VPARCEL_FROM_*) and the order of its outputs in the flags
VPARCEL_FROM = {"first": 0, "last": 1}
VPARCEL_OUTPUTS = ("cape", "cin", "plcl", "plfc", "pel", "tparcel")
# miutil::constants r and g (MetConstants.h): the gas constant of dry air, J / (kg K), and gravity, m / s^2
R_DRY, GRAVITY = 287.0, 9.8
# the methods of mifc_hinterp_levels (MIFC_HINTERP_*)
HINTERP_METHODS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
# the modes and product groups of mifc_hstats_levels (MIFC_HSTATS_*)
HSTATS_MODES = {"area": 0, "rows": 1}
HSTATS_PRODUCTS = {"moments": 1, "extremes": 2}
# the operations of mifc_fexpr_levels (MIFC_FEXPR_*, in enum order), where its operand bytes begin and its limits
FEXPR_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "min": 4, "max": 5, "abs": 6, "neg": 7, "sqrt": 8, "log": 9, "log10": 10, "exp": 11, "pow10": 12,
             "pow": 13, "lt": 14, "le": 15, "eq": 16, "ne": 17, "select": 18, "ifdef": 19, "mask": 20, "mov": 21}
FEXPR_LEVEL0, FEXPR_CONST0 = 16, 32
FEXPR_LIMITS = {"nregs": 16, "fields": 8, "planes": 4, "inputs": 12, "scalars": 4, "consts": 16, "code": 64, "out": 4}
