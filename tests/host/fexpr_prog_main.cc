// The program check of mi-fieldcalc_amd/csrc/mifc_fexpr_prog.h as a stand-alone host program (no device code):
// tests/test_fexpr_cpu.py builds it with -fsanitize=address,undefined and runs it.  The cases are the ones of that test:
// every refusal once, with arrays of exactly the size the check may read (heap vectors: the address sanitizer sees a read
// past them), and valid programs at the limits -- 64 instructions, 16 registers, 12 inputs.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mifc_fexpr_prog.h"

namespace {

int failures = 0, cases = 0;

struct Case
{
  int nfields = 2, nplanes = 1, nscalars = 1, nconsts = 1;
  std::vector<mifc_fexpr_ins> code;
  std::vector<int> out_regs;
  int ncode = -1, nout = -1; // -1: the size of the vector
  bool null_code = false, null_out = false;
};

mifc_fexpr_ins ins(int op, int dst, int a, int b = 0, int c = 0)
{
  mifc_fexpr_ins w;
  std::memset(&w, 0, sizeof w);
  w.op = (unsigned char)op;
  w.dst = (unsigned char)dst;
  w.a = (unsigned char)a;
  w.b = (unsigned char)b;
  w.c = (unsigned char)c;
  return w;
}

Case base()
{
  Case k;
  k.code.push_back(ins(MIFC_FEXPR_ADD, 3, 0, 1));
  k.out_regs.push_back(3);
  return k;
}

int run(const Case& k, mifc_fexpr::Program* prog, char* why, size_t n)
{
  return mifc_fexpr::check(k.nfields, k.nplanes, k.nscalars, k.nconsts, k.null_code ? nullptr : k.code.data(), k.ncode < 0 ? (int)k.code.size() : k.ncode,
                           k.null_out ? nullptr : k.out_regs.data(), k.nout < 0 ? (int)k.out_regs.size() : k.nout, prog, why, n);
}

void refused(const Case& k, const char* needle)
{
  mifc_fexpr::Program prog;
  char why[128] = "";
  cases += 1;
  if (run(k, &prog, why, sizeof why) != 0 || !std::strstr(why, needle)) {
    std::fprintf(stderr, "case %d: expected a refusal with \"%s\", got \"%s\"\n", cases, needle, why);
    failures += 1;
  }
}

void accepted(const Case& k, int nregs, int tables)
{
  mifc_fexpr::Program prog;
  char why[128] = "";
  cases += 1;
  if (run(k, &prog, why, sizeof why) != 1 || prog.nregs != nregs || prog.tables != tables || why[0] != 0) {
    std::fprintf(stderr, "case %d: expected nregs %d tables %d, got \"%s\" nregs %d tables %d\n", cases, nregs, tables, why, prog.nregs, prog.tables);
    failures += 1;
  }
}

} // namespace

int main()
{
  Case k;
  accepted(base(), 4, 0);
  // the counts
  k = base(), k.nfields = 9, refused(k, "nfields 9 outside");
  k = base(), k.nfields = -1, refused(k, "nfields -1 outside");
  k = base(), k.nplanes = 5, refused(k, "nplanes 5 outside");
  k = base(), k.nfields = 0, k.nplanes = 0, refused(k, "nfields + nplanes 0 outside");
  k = base(), k.nscalars = 5, refused(k, "nscalars 5 outside");
  k = base(), k.nconsts = 17, refused(k, "nconsts 17 outside");
  k = base(), k.ncode = 0, refused(k, "ncode 0 outside");
  k = base(), k.ncode = 65, refused(k, "ncode 65 outside");
  k = base(), k.nout = 0, refused(k, "nout 0 outside");
  k = base(), k.nout = 5, refused(k, "nout 5 outside");
  k = base(), k.null_code = true, refused(k, "null pointer");
  k = base(), k.null_out = true, refused(k, "null pointer");
  // the instructions
  k = base(), k.code[0].op = MIFC_FEXPR_NOPS, refused(k, "unknown op 22");
  k = base(), k.code[0].dst = 16, refused(k, "dst 16 is no register");
  k = base(), k.code[0].b = 20, refused(k, "operand byte 20");
  k = base(), k.code[0].b = 200, refused(k, "operand byte 200");
  k = base(), k.code[0].b = MIFC_FEXPR_LEVEL(1), refused(k, "level scalar 1 out of range");
  k = base(), k.code[0].a = MIFC_FEXPR_CONST(1), refused(k, "constant 1 out of range");
  k = base(), k.code[0].b = 5, refused(k, "register 5 is read before");
  k = base(), k.code[0] = ins(MIFC_FEXPR_SELECT, 3, 0, 1, 9), refused(k, "register 9 is read before");
  k = base(), k.code[0] = ins(MIFC_FEXPR_MASK, 3, 0, 200, 9), refused(k, "register 9 is read before");
  // out_regs
  k = base(), k.out_regs[0] = 7, refused(k, "out_regs[0]: register 7 is read before");
  k = base(), k.out_regs[0] = 16, refused(k, "out_regs[0] = 16 is no register");
  k = base(), k.out_regs[0] = -1, refused(k, "out_regs[0] = -1 is no register");
  // accepted: bytes an operation does not read are ignored, and come back as `a`
  {
    k = base();
    k.code[0] = ins(MIFC_FEXPR_ABS, 3, 1, 200, 77);
    k.code.push_back(ins(MIFC_FEXPR_MASK, 4, 3, 201, MIFC_FEXPR_LEVEL(0)));
    k.code.push_back(ins(MIFC_FEXPR_POW, 5, 4, MIFC_FEXPR_CONST(0), 99));
    k.out_regs[0] = 5;
    accepted(k, 6, 1);
    mifc_fexpr::Program prog;
    char why[128];
    cases += 1;
    if (!run(k, &prog, why, sizeof why) || prog.code[0].b != 1 || prog.code[0].c != 1 || prog.code[1].b != 3 || prog.code[1].c != MIFC_FEXPR_LEVEL(0) ||
        prog.code[2].b != MIFC_FEXPR_CONST(0) || prog.code[2].c != 4 || prog.out_regs[0] != 5) {
      std::fprintf(stderr, "case %d: the normalised program\n", cases);
      failures += 1;
    }
  }
  // the limits: 12 inputs, 16 registers, 64 instructions, 4 outputs, every operand kind at its last index
  {
    k = Case();
    k.nfields = 8, k.nplanes = 4, k.nscalars = 4, k.nconsts = 16;
    for (int i = 0; i < 64; ++i)
      k.code.push_back(ins(i % MIFC_FEXPR_NOPS, 12 + i % 4, i % 12, i % 2 ? MIFC_FEXPR_LEVEL(3) : MIFC_FEXPR_CONST(15), 11));
    k.out_regs = {12, 13, 14, 15};
    accepted(k, 16, 1);
  }
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
