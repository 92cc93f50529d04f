// mifc_fexpr_prog.h -- the program check of mifc_fexpr_levels (include/mifc.h, rules 1, 2, 5 and 6): the counts, the
// ranges of every byte an instruction reads, set-before-read, and the registers in use.  Host code only, nothing of the
// device runtime: the host compiler builds it alone (tests/fexpr_prog_shim.cc, tests/host/fexpr_prog_main.cc).
// The checked program comes back normalised for the kernel: the source bytes an operation does not read repeat `a`, so the
// interpreter may fetch and test them without a case per operation.
#ifndef MIFC_FEXPR_PROG_H
#define MIFC_FEXPR_PROG_H

#include "../../include/mifc.h"

#include <cstdio>

namespace mifc_fexpr {

// what an operation reads: 1 = a, 2 = a and b, 3 = a, b and c, 4 = a and c (MASK)
inline int reads(int op)
{
  switch (op) {
  case MIFC_FEXPR_ABS:
  case MIFC_FEXPR_NEG:
  case MIFC_FEXPR_SQRT:
  case MIFC_FEXPR_LOG:
  case MIFC_FEXPR_LOG10:
  case MIFC_FEXPR_EXP:
  case MIFC_FEXPR_POW10:
  case MIFC_FEXPR_MOV:
    return 1;
  case MIFC_FEXPR_SELECT:
    return 3;
  case MIFC_FEXPR_MASK:
    return 4;
  default:
    return 2;
  }
}

inline bool needs_tables(int op)
{
  return op == MIFC_FEXPR_LOG || op == MIFC_FEXPR_LOG10 || op == MIFC_FEXPR_EXP || op == MIFC_FEXPR_POW10 || op == MIFC_FEXPR_POW;
}

struct Program
{
  mifc_fexpr_ins code[MIFC_FEXPR_MAX_CODE]; // normalised
  unsigned char out_regs[MIFC_FEXPR_MAX_OUT];
  int ncode, nout;
  int nregs;  // the registers in use: the highest register set or read, plus one
  int tables; // an operation needs the log2 / exp2 tables
};

// 1, or 0 with the reason in `why`.  The counts first, then the instructions in order, then out_regs.
inline int check(int nfields, int nplanes, int nscalars, int nconsts, const mifc_fexpr_ins* code, int ncode, const int* out_regs, int nout, Program* prog,
                 char* why, size_t why_len)
{
  auto no = [&](const char* fmt, int x = 0, int y = 0) {
    std::snprintf(why, why_len, fmt, x, y);
    return 0;
  };
  if (nfields < 0 || nfields > MIFC_FEXPR_MAX_FIELDS)
    return no("nfields %d outside 0..%d", nfields, MIFC_FEXPR_MAX_FIELDS);
  if (nplanes < 0 || nplanes > MIFC_FEXPR_MAX_PLANES)
    return no("nplanes %d outside 0..%d", nplanes, MIFC_FEXPR_MAX_PLANES);
  if (nfields + nplanes < 1 || nfields + nplanes > MIFC_FEXPR_MAX_INPUTS)
    return no("nfields + nplanes %d outside 1..%d", nfields + nplanes, MIFC_FEXPR_MAX_INPUTS);
  if (nscalars < 0 || nscalars > MIFC_FEXPR_MAX_SCALARS)
    return no("nscalars %d outside 0..%d", nscalars, MIFC_FEXPR_MAX_SCALARS);
  if (nconsts < 0 || nconsts > MIFC_FEXPR_MAX_CONSTS)
    return no("nconsts %d outside 0..%d", nconsts, MIFC_FEXPR_MAX_CONSTS);
  if (ncode < 1 || ncode > MIFC_FEXPR_MAX_CODE)
    return no("ncode %d outside 1..%d", ncode, MIFC_FEXPR_MAX_CODE);
  if (nout < 1 || nout > MIFC_FEXPR_MAX_OUT)
    return no("nout %d outside 1..%d", nout, MIFC_FEXPR_MAX_OUT);
  if (!code || !out_regs)
    return no("a null pointer (code or out_regs)");

  unsigned int set = (1u << (nfields + nplanes)) - 1u; // bit r: register r holds something
  int top = nfields + nplanes;
  prog->tables = 0;
  for (int i = 0; i < ncode; ++i) {
    mifc_fexpr_ins w = code[i];
    if (w.op >= MIFC_FEXPR_NOPS)
      return no("instruction %d: unknown op %d", i, w.op);
    const int r = reads(w.op);
    const unsigned char src[3] = {w.a, r == 2 || r == 3 ? w.b : w.a, r >= 3 ? w.c : w.a};
    for (int s = 0; s < 3; ++s) {
      const int x = src[s];
      if (x < MIFC_FEXPR_NREGS) {
        if (!((set >> x) & 1u))
          return no("instruction %d: register %d is read before anything set it", i, x);
        top = x + 1 > top ? x + 1 : top;
      } else if (x >= MIFC_FEXPR_LEVEL(0) && x < MIFC_FEXPR_LEVEL(MIFC_FEXPR_MAX_SCALARS)) {
        if (x - MIFC_FEXPR_LEVEL(0) >= nscalars)
          return no("instruction %d: level scalar %d out of range", i, x - MIFC_FEXPR_LEVEL(0));
      } else if (x >= MIFC_FEXPR_CONST(0) && x < MIFC_FEXPR_CONST(MIFC_FEXPR_MAX_CONSTS)) {
        if (x - MIFC_FEXPR_CONST(0) >= nconsts)
          return no("instruction %d: constant %d out of range", i, x - MIFC_FEXPR_CONST(0));
      } else {
        return no("instruction %d: operand byte %d is no register, level scalar or constant", i, x);
      }
    }
    if (w.dst >= MIFC_FEXPR_NREGS)
      return no("instruction %d: dst %d is no register", i, w.dst);
    set |= 1u << w.dst;
    top = w.dst + 1 > top ? w.dst + 1 : top;
    prog->tables |= needs_tables(w.op) ? 1 : 0;
    w.a = src[0];
    w.b = src[1];
    w.c = src[2];
    w.pad[0] = w.pad[1] = w.pad[2] = 0;
    prog->code[i] = w;
  }
  for (int o = 0; o < nout; ++o) {
    if (out_regs[o] < 0 || out_regs[o] >= MIFC_FEXPR_NREGS)
      return no("out_regs[%d] = %d is no register", o, out_regs[o]);
    if (!((set >> out_regs[o]) & 1u))
      return no("out_regs[%d]: register %d is read before anything set it", o, out_regs[o]);
    prog->out_regs[o] = (unsigned char)out_regs[o];
  }
  for (int o = nout; o < MIFC_FEXPR_MAX_OUT; ++o)
    prog->out_regs[o] = prog->out_regs[0];
  prog->ncode = ncode;
  prog->nout = nout;
  prog->nregs = top;
  if (why_len)
    why[0] = 0;
  return 1;
}

} // namespace mifc_fexpr

#endif // MIFC_FEXPR_PROG_H
