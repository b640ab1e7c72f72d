// The instantiations of the on-chip CG kernel that live outside persist.o: one row list of persist_shapes.h and its lookup,
// compiled once per object with -DMAG_PERSIST_LIST=K4, CASES or VARIANTS (Makefile; the lists say why each has an object).
#include "persist_kernel.h"
#include "persist_shapes.h"

#define MAG_PERSIST_CAT_(A_, B_) A_##B_
#define MAG_PERSIST_CAT(A_, B_) MAG_PERSIST_CAT_(A_, B_)

namespace magk {

PersistKernel MAG_PERSIST_CAT(persist_kernel_, MAG_PERSIST_LIST)(const PersistShape &sh)
{
#define MAG_PERSIST_ROW(...) MAG_PERSIST_ROW_KERNEL(MAG_PERSIST_CAT(MAG_PERSIST_MEMBERS_, MAG_PERSIST_LIST), __VA_ARGS__)
    MAG_PERSIST_CAT(MAG_PERSIST_ROWS_, MAG_PERSIST_LIST)(MAG_PERSIST_ROW)
#undef MAG_PERSIST_ROW
    return nullptr;
}

} // namespace magk
