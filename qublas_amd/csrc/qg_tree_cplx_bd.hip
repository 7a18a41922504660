// qg_tree_cplx_bd.hip — the batched twins of qg_tree_cplx.hip's 12-level kernels (QG_OPT_BATCHED_TREE): that file's text compiled again
// behind the walk over the members (qg_tree_bd.h), every form qg_launch_tree_cplx_fast serves; it ends in qg_launch_tree_cplx_fast_bd.
#define QG_TREE_BD 1
#include "qg_tree_cplx.hip"
