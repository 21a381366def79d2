// k7_decode_windows.hip -- K7's window mode: of every segment of a batch only a window of samples is delivered, the
// windows back to back in pcm.  k_decode_frames_windows and k_decode_windows are the window instances of k7_frame.h's two
// passes (see there), launched by launch_decode_windows; k7_decode.hip's launch_decode_end ends the batch.
#include "k7_frame.h"

namespace fhip {
namespace {

__global__ void __launch_bounds__(DHDR_T) k_decode_frames_windows(DecodeWindowArgs w) { decode_frames<true, true>(w.d, &w); }

__global__ void __launch_bounds__(DT) k_decode_windows(DecodeWindowArgs w) { decode_frame_window(w.d, w.clip); }

}  // namespace

hipError_t launch_decode_windows(hipStream_t st, const DecodeWindowArgs &w)
{
    const DecodeArgs &a = w.d;
    if (!decode_segments_ok(a) || !w.seg_skip || !w.seg_take || (a.nframes > 0 && !w.clip)) return hipErrorInvalidValue;
    note_launch("k_decode_frames windows");
    hipLaunchKernelGGL(k_decode_frames_windows, dim3(1), dim3(DHDR_T), 0, st, w);
    if (a.nframes > 0) {
        note_launch("k_decode windows");
        hipLaunchKernelGGL(k_decode_windows, dim3(a.nframes), dim3(DT), 0, st, w);
    }
    return launch_decode_end(st, a);
}

}  // namespace fhip
