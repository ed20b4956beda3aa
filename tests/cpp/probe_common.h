// probe_common.h — what the kernel probes share beyond the container: the checked HIP call, and the driver of the three role-buffer probes
// (DESIGN.md "Probe container").  gemm_probe.hip has its own file format and takes HIP_OK, Reader and the patterns only.
#pragma once
#include "probe_case.h"
#include <hip/hip_runtime.h>

#define HIP_OK(call)                                                                                        \
    do {                                                                                                    \
        const hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            std::fprintf(stderr, "%s: %s -> %s (%s:%d)\n", probe_program, #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            std::fflush(stdout);                                                                            \
            std::exit(3);                                                                                   \
        }                                                                                                   \
    } while (0)

// what follows every launch: its error, then the stream's
inline void launched(hipStream_t s) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(s));
}

// main() of a role-buffer probe.  validate(c) refuses a case the kernels must not see; launch(c, s) makes the case's launch or launches, each
// followed by launched(s); fields(c) prints the case's JSON fields behind {"case": "<name>".  A case's line is printed, and flushed, only
// after its results are in the file: the number of lines says which case was running when a process ended early.
template <class C, class Validate, class Launch, class Fields>
int probe_main(int argc, char **argv, const ProbeSpec &spec, Validate validate, Launch launch, Fields fields) {
    probe_program = spec.program;
    if (argc != 3) { std::fprintf(stderr, "usage: %s <cases.bin> <results.bin>\n", spec.program); return 2; }
    std::vector<C> cases = read_case_file<C>(argv[1], spec);
    for (C &c : cases) validate(c);                                    // all of them, before the GPU is touched

    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) { std::fprintf(stderr, "%s: cannot write %s\n", spec.program, argv[2]); return 2; }
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    for (C &c : cases) {
        for (Buf &x : c.b) {
            HIP_OK(hipMalloc(&x.dev, x.nbytes));
            HIP_OK(hipMemcpy(x.dev, x.host.data(), x.nbytes, hipMemcpyHostToDevice));
        }
        launch(c, s);
        for (Buf &x : c.b) {
            if (x.flags & 1) {
                HIP_OK(hipMemcpy(x.host.data(), x.dev, x.nbytes, hipMemcpyDeviceToHost));
                if (std::fwrite(x.host.data(), 1, x.nbytes, fo) != (size_t)x.nbytes) bad_file("short write");
            }
            HIP_OK(hipFree(x.dev));
            x.dev = nullptr;
            std::vector<uint8_t>().swap(x.host);
        }
        std::printf("{\"case\": \"%s\"", c.name.c_str());
        fields(c);
        std::printf("}\n");
        std::fflush(stdout);
    }
    HIP_OK(hipStreamDestroy(s));
    if (std::fclose(fo) != 0) bad_file("close failed");
    return 0;
}
