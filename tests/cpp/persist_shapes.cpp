// The row lists of persist_shapes.h and persist_shape's answer over a small domain, as text for tests/test_persist_shapes.py.
// Host compiler only: the header has no HIP type in it.
#include <cstdio>

#include "persist_shapes.h"

using namespace magk;

int main()
{
#define ROW(B_, MG_, EBM_, ONE_, NPTX_) printf("row %s %d %d %d %d %d\n", list, (int)B_, (int)MG_, (int)EBM_, (int)ONE_, (int)NPTX_);
    const char *list = "main";
    MAG_PERSIST_ROWS_MAIN(ROW)
    list = "k4";
    MAG_PERSIST_ROWS_K4(ROW)
    list = "cases";
    MAG_PERSIST_ROWS_CASES(ROW)
    list = "variants";
    MAG_PERSIST_ROWS_VARIANTS(ROW)
#undef ROW
    const int Bs[2] = {256, 512}, ranks[3] = {1, 2, 8};
    const PersistMembers kinds[3] = {PERSIST_SINGLE, PERSIST_CASES, PERSIST_VARIANTS};
    for (int B : Bs)
        for (int R : ranks)
            for (int grid = 1; grid <= 3; ++grid)
                for (int k = 1; k <= 2048 / B; ++k)
                    for (int eb = 0; eb <= 2; ++eb)
                        for (PersistMembers m : kinds) {
                            PersistShape sh = {};
                            const bool ok = persist_shape(B, R, grid, k, eb, m, sh);
                            printf("shape %d %d %d %d %d %d :", B, R, grid, k, eb, (int)m);
                            if (ok)
                                printf(" %d %d %d %d %d %d\n", (int)sh.B, (int)sh.mg, sh.ebm, (int)sh.one, sh.nptx, (int)sh.members);
                            else
                                printf(" none\n");
                        }
    return 0;
}
