// uda_tta_fuse for TTA_FUSE_A_LAST + 1..TTA_FUSE_B_LAST views (tta_fuse.h says why there are three of these)
#include "tta_fuse.h"

TTA_FUSE_PIECE(tta_fuse_launch_b, TTA_FUSE_A_LAST + 1, TTA_FUSE_B_LAST)
