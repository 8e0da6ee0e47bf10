// context_adapter_kernels.hip -- TOOL ONLY (tools/context_binding_timing.py, leg A): the three kernels the OpenMM adapter
// (integration/openmm_hip/HipNonbondedSlicingKernels.cpp) launched around every snb_execute before the engine could be bound to the
// context's own buffers (snb_bind_context) -- posq in context order -> user-order positions, user-order forces -> the context's 64-bit
// fixed-point buffer (three atomics per atom), raw slice energies -> the derivative buffer -- kept here, as they were, so that what they cost
// can be measured against the bound engine.  Not part of the product.
//   hipcc -O3 -fPIC -shared --offload-arch=gfx950 tools/context_adapter_kernels.hip -o tools_out/libcontext_adapter_kernels.so
#include <hip/hip_runtime.h>

template <typename Real>
__global__ void addForcesToContext(const Real* __restrict__ forces, const int* __restrict__ atomIndex, unsigned long long* __restrict__ forceBuffers,
                                   int numAtoms, int paddedNumAtoms) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= numAtoms) return;
    const int user = atomIndex[slot];
    const double scale = 4294967296.0;
    for (int d = 0; d < 3; d++)
        atomicAdd(&forceBuffers[slot + d * (size_t)paddedNumAtoms], (unsigned long long)(long long)((double)forces[3 * (size_t)user + d] * scale));
}

template <typename Mixed>
__global__ void addDerivativesToContext(const double* __restrict__ sliceEnergies, const int* __restrict__ binding, int n, Mixed* __restrict__ derivBuffer) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && binding[k] >= 0) atomicAdd(&derivBuffer[binding[k]], (Mixed)sliceEnergies[k]);
}

template <typename Real4>
__global__ void gatherUserPositions(const Real4* __restrict__ posq, const int* __restrict__ atomIndex, Real4* __restrict__ userPos, int numAtoms) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= numAtoms) return;
    userPos[atomIndex[slot]] = posq[slot];
}

extern "C" {
void adapter_gather_positions(const void* posq, const int* atomIndex, void* userPos, int n, int isDouble, void* stream) {
    const int blocks = (n + 255) / 256;
    if (isDouble) hipLaunchKernelGGL(gatherUserPositions<double4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const double4*)posq, atomIndex, (double4*)userPos, n);
    else hipLaunchKernelGGL(gatherUserPositions<float4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)posq, atomIndex, (float4*)userPos, n);
}
void adapter_add_forces(const void* forces, const int* atomIndex, void* forceBuffers, int n, int paddedN, int isDouble, void* stream) {
    const int blocks = (n + 255) / 256;
    if (isDouble) hipLaunchKernelGGL(addForcesToContext<double>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const double*)forces, atomIndex, (unsigned long long*)forceBuffers, n, paddedN);
    else hipLaunchKernelGGL(addForcesToContext<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)forces, atomIndex, (unsigned long long*)forceBuffers, n, paddedN);
}
void adapter_add_derivatives(const double* sliceEnergies, const int* binding, int n, void* derivBuffer, int isDouble, void* stream) {
    if (isDouble) hipLaunchKernelGGL(addDerivativesToContext<double>, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, sliceEnergies, binding, n, (double*)derivBuffer);
    else hipLaunchKernelGGL(addDerivativesToContext<float>, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, sliceEnergies, binding, n, (float*)derivBuffer);
}
}
