// uda_tta_fuse for 2..TTA_FUSE_A_LAST views (tta_fuse.h says why there are three of these)
#include "tta_fuse.h"

TTA_FUSE_PIECE(tta_fuse_launch_a, 2, TTA_FUSE_A_LAST)
