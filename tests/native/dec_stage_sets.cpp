// Whether the table-driven decode kernel can run a survivor set: compile_pattern's rule (engine.cpp)
// restated over ClayHost -- the padded erasure pattern of every stripe must compile to a plane
// program (dec_prog, either row orientation) that fits the kernel's LDS rows and packs into
// DecStepP steps; one pattern without one sends the whole call to the generic kernel.
// Usage: dec_stage_sets n k d < lines of "avail_mask(hex) lost_slice(-1: decode) stripes rotated";
// prints 1 or 0 per line.  tests/test_decode_geometry_cases.py pins the GPU tests' case tables with it.
#include <cstdio>
#include <cstdlib>
#include "clay_host.hpp"
using namespace tec;

static bool staged(const ClayHost &h, uint64_t emask, int out_node) {
    GpePattern P;
    std::vector<uint16_t> planes;
    if (!h.gpe_pattern(emask, P, planes)) return false;
    if (h.k < 7 || h.k > 10 || P.nknown != (uint32_t)h.k || P.nerased != (uint32_t)(h.n - h.k)) return false;
    for (int orient = 0; orient < 2; orient++) {
        DecProgHdr H;
        std::vector<DecStep> st;
        if (!h.dec_prog(P, orient, H, st, out_node) || 2 + H.nslots > 64) continue;  // decode_stage_fits, direct output
        bool ok = true;
        for (const DecStep &S : st) {
            DecStepP p;
            ok = ok && ClayHost::dec_pack(S, p);
        }
        if (ok) return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    ClayHost h;
    if (h.init(atoi(argv[1]), atoi(argv[2]), atoi(argv[3])) != 0) return 2;
    unsigned avail;
    int lost, stripes, rotated;
    while (scanf("%x %d %d %d", &avail, &lost, &stripes, &rotated) == 4) {
        bool all = true;
        for (int st = 0; st < stripes; st++) {
            const int off = rotated ? (st * 7) % h.n : 0;
            uint64_t em = 0;
            for (int sh = 0; sh < h.n; sh++)
                if (!((avail >> ((sh + off) % h.n)) & 1u)) em |= 1ull << h.ext_to_int(sh);
            em = h.pad_erasures(em);
            const int onode = lost < 0 ? -1 : h.ext_to_int((lost + h.n - off) % h.n);
            all = all && staged(h, em, onode);
        }
        printf("%d\n", all ? 1 : 0);
    }
    return 0;
}
