/* The gfx950 code object of vgpu-validate (src/kernels/validate_kernels.hip), embedded as
   read-only data: VGPU_VALIDATE_CO is the path of the compiled ELF. */
    .section .rodata
    .balign 4096
    .globl vgpu_validate_co
    .globl vgpu_validate_co_end
vgpu_validate_co:
    .incbin VGPU_VALIDATE_CO
vgpu_validate_co_end:
    .byte 0
    .section .note.GNU-stack,"",@progbits
