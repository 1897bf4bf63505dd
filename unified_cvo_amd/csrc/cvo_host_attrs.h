// cvo_host_attrs.h -- lets a host compiler take the headers that kernels and plain C++ share (cvo_bki_math.h, cvo_pose_math.h):
// without hipcc the two function attributes are empty.
#pragma once
#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
