// The program check of mifc_fexpr_levels (mi-fieldcalc_amd/csrc/mifc_fexpr_prog.h) behind a C entry, built by the host
// compiler alone for tests/test_fexpr_cpu.py.
#include "mifc_fexpr_prog.h"

#include <cstring>

extern "C" {

// code: ncode rows of 8 bytes; info: int[2] = nregs, tables; norm: ncode * 8 bytes, the normalised program; 1 or 0 + why
int mifc_test_fexpr_check(int nfields, int nplanes, int nscalars, int nconsts, const unsigned char* code, int ncode, const int* out_regs, int nout,
                          int* info, unsigned char* norm, char* why, int why_len)
{
  static_assert(sizeof(mifc_fexpr_ins) == 8, "an instruction is 8 bytes");
  mifc_fexpr::Program prog;
  const int ok = mifc_fexpr::check(nfields, nplanes, nscalars, nconsts, reinterpret_cast<const mifc_fexpr_ins*>(code), ncode, out_regs, nout, &prog, why,
                                   (size_t)why_len);
  if (ok) {
    info[0] = prog.nregs;
    info[1] = prog.tables;
    std::memcpy(norm, prog.code, (size_t)ncode * sizeof(mifc_fexpr_ins));
  }
  return ok;
}

} // extern "C"
