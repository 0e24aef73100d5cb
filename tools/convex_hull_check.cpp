// Stand-alone check of the host hull builder (nellie_amd/csrc/convex_hull.h) for the host sanitizers; tools/convex_hull_check.py
// writes its input, compiles it with -fsanitize=address,undefined and runs it.
//
//     convex_hull_check FILE
//
// FILE holds one region per record: "D n facets count ez ey ex" followed by n rows of D box-relative voxel coordinates (ez = 1 in
// 2-D).  For every region the facets are built, their number is compared with `facets` and the lattice points of the box that
// satisfy all of them are counted by plain loops and compared with `count`.  Exit status 0 when every region agrees.
#include <stdio.h>
#include <vector>
#include "../nellie_amd/csrc/convex_hull.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long long D, n, want_facets, want_count, ext[3];
    long long regions = 0, bad = 0;
    while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld", &D, &n, &want_facets, &want_count, &ext[0], &ext[1], &ext[2]) == 7) {
        std::vector<nl_convex::ci64> c((size_t)(n * D));
        for (auto &v : c)
            if (fscanf(f, "%lld", &v) != 1) { fprintf(stderr, "short record\n"); return 2; }
        std::vector<nl_convex::Facet> facets;
        nl_convex::ch_facets(c.data(), n, (int)D, facets);
        long long count = 0;
        if (!facets.empty())
            for (long long z = 0; z < ext[0]; ++z)
                for (long long y = 0; y < ext[1]; ++y)
                    for (long long x = 0; x < ext[2]; ++x) {
                        bool in = true;
                        for (const nl_convex::Facet &k : facets) in = in && k.nz * 2 * z + k.ny * 2 * y + k.nx * 2 * x <= k.d;
                        count += in;
                    }
        ++regions;
        if ((long long)facets.size() != want_facets || count != want_count) {
            ++bad;
            fprintf(stderr, "region %lld: %zu facets (want %lld), count %lld (want %lld)\n", regions, facets.size(), want_facets, count, want_count);
        }
    }
    fclose(f);
    printf("%lld regions, %lld differ\n", regions, bad);
    return bad || !regions ? 1 : 0;
}
