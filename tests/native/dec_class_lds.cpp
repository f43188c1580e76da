// LDS need of every decode / recover class kernel (dec_class.hpp): the slot and scratch row counts
// of each class program and the per-call kernel's ring rows (dec_class_source's nring_out: the
// values the generated kernel registers and launch_dec_class sizes its dynamic LDS from), and
// dec_class_lds() of them for the per-call kernel (G = 1: ring, slot and scratch rows all in LDS)
// and the batch kernel (G = 2: slot rows).  One class per line: id nslots nscratch nring lds(G=1)
// lds(G=2).  tests/test_dec_class_host.py asserts that every figure fits a gfx950 workgroup's LDS,
// so a class that does not fit fails on the CPU, not as a launch error.
#include <cstdio>
#include <string>
#include "dec_class.hpp"
using namespace tec;

int main() {
    ClayHost h;
    if (h.init(20, 7, 16) != 0) return 2;
    for (int id = 0; id < kDecClasses; id++) {
        DecProgHdr H{};
        uint32_t nring = 0;
        if (dec_class_source(h, id, kPft.t_u[0], H, DecClassGenOpt(), &nring).empty() || nring < 1) return 1;
        printf("%d %u %u %u %zu %zu\n", id, H.nslots, H.nscratch, nring, dec_class_lds(H.nslots, H.nscratch, nring, 1),
               dec_class_lds(H.nslots, H.nscratch, nring, 2));
    }
    return 0;
}
