"""The reference's own functions, one 2-D field at a time: operator names, argument order and failure behaviour follow
``miutil::fieldcalc`` -- where the C++ function returns ``false`` the method returns ``None``."""
import ctypes

import numpy as np

from ._args import _Arg, _empty_like, _kept, _pointer_table, _same_shape
from ._consts import ALL_DEFINED, SOME_DEFINED, UNDEF


class _ReferenceOps:
    """Mixin of Context: the elementwise, stencil, catalogue, ensemble, neighbourhood and icing functions on (ny, nx) fields."""

    @staticmethod
    def _nxny(a):
        ny, nx = a.shape[-2], a.shape[-1]
        return nx, ny

    def _single(self, name, fields, scalars, outs, fdefined, undef, n_out=1, out_like=None, lead=(), pre=(), tail=()):
        """fields: input arrays (None allowed), scalars: list placed between
        inputs and outputs in reference order, outs: preallocated or None.
        lead: arguments before (nx, ny) (fieldOPER*'s compute), pre: scalars
        before the fields, tail: arguments between the outputs and the flag."""
        fa = [_Arg(f, allow_none=True) for f in fields]
        ref = next(f for f in fields if f is not None)
        ra = _Arg(ref)
        if len(ra.shape) != 2:
            return None  # like the reference's binding (py_mi_fieldcalc.cc:82-83): not a 2-D field
        nx, ny = self._nxny(ra)
        outs = list(outs)
        for k in range(n_out):
            if outs[k] is None:
                outs[k] = _empty_like(ref)
        oa = [_Arg(o, output=True) for o in outs]
        # every field of the call has the shape of the first one; the reference's binding returns None
        # otherwise (same_dims, py_mi_fieldcalc.cc:82-83) -- here it also keeps the kernels inside the buffers
        if not _same_shape(fa + oa, ra.shape):
            return None
        fd = ctypes.c_int(int(fdefined))
        args = (list(lead) + [nx, ny] + list(pre) + [a.addr for a in fa] + list(scalars) + [a.addr for a in oa] + list(tail)
                + [ctypes.addressof(fd), float(undef)])
        if not self._launch(name, fa + oa, args, raises=False):
            return None
        res = [_kept(o, a) for o, a in zip(outs, oa)]
        return (res[0] if n_out == 1 else tuple(res)), fd.value

    # ---------------------------------------------------- elementwise operators
    def vectorabs(self, u, v, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """ff = sqrt(u*u+v*v); FieldCalculations.cc:1819."""
        return self._single("mifc_vectorabs", [u, v], [], [out], fdefined, undef)

    def pleveltemp(self, tinp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pleveltemp", [tinp], [float(p), unit.encode(), int(compute)], [out], fdefined, undef)

    def hleveltemp(self, tinp, ps, alevel, blevel, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single(
            "mifc_hleveltemp", [tinp, ps], [float(alevel), float(blevel), unit.encode(), int(compute)], [out], fdefined, undef
        )

    def aleveltemp(self, tinp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_aleveltemp", [tinp, p], [unit.encode(), int(compute)], [out], fdefined, undef)

    def plevelhum(self, t, huminp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelhum", [t, huminp], [float(p), unit.encode(), int(compute)], [out], fdefined, undef)

    def hlevelhum(self, t, huminp, ps, alevel, blevel, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single(
            "mifc_hlevelhum", [t, huminp, ps], [float(alevel), float(blevel), unit.encode(), int(compute)], [out], fdefined, undef
        )

    def alevelhum(self, t, huminp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelhum", [t, huminp, p], [unit.encode(), int(compute)], [out], fdefined, undef)

    def cvhum(self, t, huminp, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_cvhum", [t, huminp], [unit.encode(), int(compute)], [out], fdefined, undef)

    # -------------------------------------------------------- stencil operators
    def relvort(self, u, v, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_relvort", [u, v, xmapr, ymapr], [], [out], fdefined, undef)

    def absvort(self, u, v, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_absvort", [u, v, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def divergence(self, u, v, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_divergence", [u, v, xmapr, ymapr], [], [out], fdefined, undef)

    def gradient(self, field, xmapr, ymapr, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_gradient", [field, xmapr, ymapr], [int(compute)], [out], fdefined, undef)

    def plevelgwind_xcomp(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgwind_xcomp", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def plevelgwind_ycomp(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgwind_ycomp", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def plevelgvort(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgvort", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def ilevelgwind(self, mpot, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=(None, None)):
        return self._single("mifc_ilevelgwind", [mpot, xmapr, ymapr, fcoriolis], [], list(out), fdefined, undef, n_out=2)

    # ------------------------------------------ next operators
    def advection(self, f, u, v, xmapr, ymapr, hours, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_advection", [f, u, v, xmapr, ymapr], [float(hours)], [out], fdefined, undef)

    def jacobian(self, field1, field2, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_jacobian", [field1, field2, xmapr, ymapr], [], [out], fdefined, undef)

    def momentumXcoordinate(self, v, xmapr, fcoriolis, fcoriolisMin, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_momentumXcoordinate", [v, xmapr, fcoriolis], [float(fcoriolisMin)], [out], fdefined, undef)

    def momentumYcoordinate(self, u, ymapr, fcoriolis, fcoriolisMin, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_momentumYcoordinate", [u, ymapr, fcoriolis], [float(fcoriolisMin)], [out], fdefined, undef)

    def thermalFrontParameter(self, tx, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_thermalFrontParameter", [tx, xmapr, ymapr], [], [out], fdefined, undef)

    def plevelqvector(self, z, t, xmapr, ymapr, fcoriolis, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelqvector", [z, t, xmapr, ymapr, fcoriolis], [float(p), int(compute)], [out], fdefined, undef)

    # ---------------------------- the rest of the pointwise catalogue
    # Same argument order as miutil::fieldcalc; (result, flag) or None like the others.
    def plevelthe(self, t, rh, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelthe", [t, rh], [float(p), int(compute)], [out], fdefined, undef)

    def hlevelthe(self, t, q, ps, alevel, blevel, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelthe", [t, q, ps], [float(alevel), float(blevel), int(compute)], [out], fdefined, undef)

    def alevelthe(self, t, q, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelthe", [t, q, p], [int(compute)], [out], fdefined, undef)

    def plevelducting(self, t, h, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelducting", [t, h], [float(p), int(compute)], [out], fdefined, undef)

    def hlevelducting(self, t, h, ps, alevel, blevel, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelducting", [t, h, ps], [float(alevel), float(blevel), int(compute)], [out], fdefined, undef)

    def alevelducting(self, t, h, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelducting", [t, h, p], [int(compute)], [out], fdefined, undef)

    def hlevelpressure(self, ps, alevel, blevel, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelpressure", [ps], [float(alevel), float(blevel)], [out], fdefined, undef)

    def pleveldz2tmean(self, z1, z2, p1, p2, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pleveldz2tmean", [z1, z2], [float(p1), float(p2), int(compute)], [out], fdefined, undef)

    def kIndex(self, t500, t700, rh700, t850, rh850, p500, p700, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_kIndex", [t500, t700, rh700, t850, rh850], [float(p500), float(p700), float(p850), int(compute)], [out],
                            fdefined, undef)

    def ductingIndex(self, t850, rh850, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_ductingIndex", [t850, rh850], [float(p850), int(compute)], [out], fdefined, undef)

    def showalterIndex(self, t500, t850, rh850, p500, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_showalterIndex", [t500, t850, rh850], [float(p500), float(p850), int(compute)], [out], fdefined, undef)

    def boydenIndex(self, t700, z700, z1000, p700, p1000, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_boydenIndex", [t700, z700, z1000], [float(p700), float(p1000), int(compute)], [out], fdefined, undef)

    def sweatIndex(self, t850, t500, td850, td500, u850, v850, u500, v500, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_sweatIndex", [t850, t500, td850, td500, u850, v850, u500, v500], [], [out], fdefined, undef)

    def seaSoundSpeed(self, t, s, z, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_seaSoundSpeed", [t, s], [float(z), int(compute)], [out], fdefined, undef)

    def cvtemp(self, tinp, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_cvtemp", [tinp], [int(compute)], [out], fdefined, undef)

    def abshum(self, t, rhum, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_abshum", [t, rhum], [], [out], fdefined, undef)

    def windCooling(self, t, u, v, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_windCooling", [t, u, v], [int(compute)], [out], fdefined, undef)

    def underCooledRain(self, precip, snow, tk, precipMin, snowRateMax, tcMax, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_underCooledRain", [precip, snow, tk], [float(precipMin), float(snowRateMax), float(tcMax)], [out], fdefined, undef)

    def pressure2FlightLevel(self, pressure, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pressure2FlightLevel", [pressure], [], [out], fdefined, undef)

    def snow_in_cm(self, snow_water, tk2m, td2m, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_snow_in_cm", [snow_water, tk2m, td2m], [], [out], fdefined, undef)

    def values2classes(self, fvalue, values, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """values: the class limits (host sequence).  C order: fvalue, fclass (output), values, nvalues."""
        vals = np.ascontiguousarray(values, dtype=np.float32)
        return self._single("mifc_values2classes", [fvalue], [], [out], fdefined, undef, tail=[vals.ctypes.data, int(vals.size)])

    def shapiro2_filter(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """Second-order Shapiro filter; pass out=field to smooth in place."""
        return self._single("mifc_shapiro2_filter", [field], [], [out], fdefined, undef)

    def vesselIcingOverland(self, airtemp, seatemp, u, v, sal, aice, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_vesselIcingOverland", [airtemp, seatemp, u, v, sal, aice], [], [out], fdefined, undef)

    def vesselIcingMertins(self, airtemp, seatemp, u, v, sal, aice, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_vesselIcingMertins", [airtemp, seatemp, u, v, sal, aice], [], [out], fdefined, undef)

    def winddir(self, u, v, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (no reference function): meteorological wind direction, degrees the wind blows FROM,
        dd = 270 - atan2(v, u) * 180 / pi in [0, 360), calm -> 0; see include/mifc.h."""
        return self._single("mifc_winddir", [u, v], [], [out], fdefined, undef)

    def minvalueFields(self, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_minvalueFields", [field1, field2], [], [out], fdefined, undef)

    def maxvalueFields(self, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_maxvalueFields", [field1, field2], [], [out], fdefined, undef)

    def minvalueFieldConst(self, field1, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_minvalueFieldConst", [field1], [float(value)], [out], fdefined, undef)

    def maxvalueFieldConst(self, field1, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_maxvalueFieldConst", [field1], [float(value)], [out], fdefined, undef)

    def absvalueField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_absvalueField", [field], [], [out], fdefined, undef)

    def log10Field(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_log10Field", [field], [], [out], fdefined, undef)

    def pow10Field(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pow10Field", [field], [], [out], fdefined, undef)

    def logField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_logField", [field], [], [out], fdefined, undef)

    def expField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_expField", [field], [], [out], fdefined, undef)

    def powerField(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_powerField", [field], [float(value)], [out], fdefined, undef)

    def replaceUndefined(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_replaceUndefined", [field], [float(value)], [out], fdefined, undef)

    def replaceDefined(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_replaceDefined", [field], [float(value)], [out], fdefined, undef)

    def fieldOPERfield(self, compute, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_fieldOPERfield", [field1, field2], [], [out], fdefined, undef, lead=[int(compute)])

    def fieldOPERconstant(self, compute, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_fieldOPERconstant", [field], [float(value)], [out], fdefined, undef, lead=[int(compute)])

    def constantOPERfield(self, compute, value, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_constantOPERfield", [field], [], [out], fdefined, undef, lead=[int(compute)], pre=[float(value)])

    # ---------------------------------- reductions over ensemble members
    def _ensemble(self, name, fields, fdefined_in, lead, tail, fdefined, undef, out):
        """fields: sequence of member fields (all numpy or all CUDA tensors)."""
        fa = [_Arg(f) for f in fields]
        ref = fields[0] if len(fields) else out
        if ref is None:
            raise ValueError("no member fields and no output to take the shape from")
        ra = _Arg(ref)
        if len(ra.shape) != 2:
            return None
        nx, ny = self._nxny(ra)
        if out is None:
            out = _empty_like(ref)
        oa = _Arg(out, output=True)
        if not _same_shape(fa + [oa], ra.shape):
            return None
        table = _pointer_table([a.addr for a in fa], 1)
        args = list(lead) + [nx, ny, ctypes.addressof(table)]
        if fdefined_in is not None:
            flags = (ctypes.c_int * max(len(fa), 1))(*[int(x) for x in fdefined_in])
            args.append(ctypes.addressof(flags))
        fd = ctypes.c_int(int(fdefined))
        args += [len(fa)] + list(tail) + [oa.addr, ctypes.addressof(fd), float(undef)]
        if not self._launch(name, fa + [oa], args, raises=False):
            return None
        return _kept(out, oa), fd.value

    def sumFields(self, fields, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_sumFields", fields, None, [], [], fdefined, undef, out)

    def meanValue(self, fields, fdefined_in, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_meanValue", fields, fdefined_in, [], [], fdefined, undef, out)

    def stddevValue(self, fields, fdefined_in, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_stddevValue", fields, fdefined_in, [], [], fdefined, undef, out)

    def extremeValue(self, compute, fields, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_extremeValue", fields, None, [int(compute)], [], fdefined, undef, out)

    def probability(self, compute, fields, fdefined_in, limits, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        lim = np.ascontiguousarray(limits, dtype=np.float32)
        return self._ensemble("mifc_probability", fields, fdefined_in, [int(compute)], [lim.ctypes.data, int(lim.size)], fdefined, undef, out)

    # ------------------------------------------------------ neighbourhood statistics
    # out=None allocates an output pre-filled with `undef`: the reference leaves some cells unwritten (neighbourFunctions:
    # interior cells that no step x step block covers; neighbourProbFunctions with range 0 and a compute other than 5 / 6:
    # every cell), and these come back as `undef` instead of uninitialised memory.  With out= given they keep its values.
    # Refusals where the reference is undefined raise RuntimeError with the reason (include/mifc.h); the reference's
    # own `false` gives None.
    def _neighbour(self, name, field, constants, compute, fdefined, undef, out):
        if out is None:
            out = _empty_like(field)
            out[...] = float(np.float32(undef))
        consts = np.ascontiguousarray(constants, dtype=np.float32).ravel()
        return self._single(name, [field], [consts.ctypes.data, int(consts.size), int(compute)], [out], fdefined, undef)

    def neighbourProbFunctions(self, field, constants, compute, fdefined=ALL_DEFINED, undef=UNDEF, out=None):
        """constants = [limit, range]; compute 5: fraction of the (2r+1)^2 box above limit, 6: below.  out=field works in place."""
        return self._neighbour("mifc_neighbourProbFunctions", field, constants, compute, fdefined, undef, out)

    def neighbourFunctions(self, field, constants, compute, fdefined=ALL_DEFINED, undef=UNDEF, out=None):
        """compute 1 mean, 2 max, 3 min (constants = [range(, step)]), 4 percentile, 5 / 6 fraction above / below
        (constants = [percentile or limit, range(, step)]); each computed centre fills its step x step block."""
        return self._neighbour("mifc_neighbourFunctions", field, constants, compute, fdefined, undef, out)

    # ------------------------------------------------------ iterative vessel icing
    # FieldCalculationsVesselIcing.cc:182 / :677.  The reference's `false` gives None; a level count that overflows an
    # int raises RuntimeError with the reason.  out may be any input (each cell reads only its own index).
    def vesselIcingModStall(self, sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth, vs, alpha, zmin, zmax, fdefined=SOME_DEFINED,
                            undef=UNDEF, out=None):
        """Modified Stallabrass freezing-spray icing rate (cm/h)."""
        return self._single("mifc_vesselIcingModStall", [sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth],
                            [float(vs), float(alpha), float(zmin), float(zmax)], [out], fdefined, undef)

    def vesselIcingMincog(self, sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth, vs, alpha, zmin, zmax, alt, fdefined=SOME_DEFINED,
                          undef=UNDEF, out=None):
        """MINCOG icing rate (cm/h); alt == 1: MINCOG org, anything else: MINCOG adj."""
        return self._single("mifc_vesselIcingMincog", [sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth],
                            [float(vs), float(alpha), float(zmin), float(zmax), int(alt)], [out], fdefined, undef)
