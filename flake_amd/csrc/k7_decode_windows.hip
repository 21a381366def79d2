// k7_decode_windows.hip -- K7's window mode: of every segment of a batch only a window of samples is delivered, the
// windows back to back in pcm.  The kernels are k7_decode.hip's text with FHIP_K7_WINDOWS set (see there):
// k_decode_frames_windows and k_decode_windows, launched by launch_decode_windows.  They stand in a file of their own so
// that k7_decode.hip goes on compiling to exactly the kernels it did.
#define FHIP_K7_WINDOWS 1
#include "k7_decode.hip"
