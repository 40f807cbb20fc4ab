// Stand-alone check of ake::launch (csrc/common.h), built and run by tests/test_launch_host.py together with csrc/common.cpp:
// one launch of an empty kernel, then the code it returned, ake_last_error() and -- for the test to compare with -- the runtime's own
// text for "no device".  On a machine without a GPU the launch is rejected, which is the branch the test is after; nothing touches memory.
#include "common.h"

__global__ void launch_check_kernel() {}

int main() {
    const int rc = ake::launch("launch_check_kernel", launch_check_kernel, dim3(1), dim3(64), 0, nullptr);
    if (rc == AKE_OK && hipDeviceSynchronize() != hipSuccess) return 1;
    std::printf("code %d\nerror %s\nno_device %s\n", rc, ake_last_error(), hipGetErrorString(hipErrorNoDevice));
    return 0;
}
