// fpq_build_tag.hip - which build this is (include/fpq.h, fpq_build_tag): "stock" for the regular build.  A unit of its own,
// so that tools/build_variant.sh can stamp a variant's name by recompiling this file, whichever unit the variant rebuilt.
#include "fpq.h"

#ifndef FPQ_BUILD_TAG
#define FPQ_BUILD_TAG "stock"
#endif
extern "C" const char* fpq_build_tag(void) { return FPQ_BUILD_TAG; }
