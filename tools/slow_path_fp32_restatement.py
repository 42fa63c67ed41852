"""CPU only: the slow path's arithmetic restated in fp32 numpy, to derive the bound of tests/test_gpu_slow_path.py::test_inverse_mass_matrix_on_random_trees.
crba32() follows rsb_query_kernel's CRBA operation by operation, kernel_restated() follows rsb_minv_kernel's loops; both run all envs of a model at once.
Prints, per model of that file: the relative error of the restated M against the oracle's, and max over envs of |Minv M_oracle - I| / (cond 2^-23)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_gpu_slow_path as T  # noqa: E402

f=np.float32
def cross(a,b): return np.stack([a[:,1]*b[:,2]-a[:,2]*b[:,1], a[:,2]*b[:,0]-a[:,0]*b[:,2], a[:,0]*b[:,1]-a[:,1]*b[:,0]],1)
def mm(A,B):  # [N,9]x[N,9]
    C=np.zeros_like(A)
    for i in range(3):
        for j in range(3): C[:,3*i+j]=A[:,3*i]*B[:,j]+A[:,3*i+1]*B[:,3+j]+A[:,3*i+2]*B[:,6+j]
    return C
def mv(A,x): return np.stack([A[:,3*i]*x[:,0]+A[:,3*i+1]*x[:,1]+A[:,3*i+2]*x[:,2] for i in range(3)],1)
def dot6(a,b): return a[:,0]*b[:,0]+a[:,1]*b[:,1]+a[:,2]*b[:,2]+a[:,3]*b[:,3]+a[:,4]*b[:,4]+a[:,5]*b[:,5]
def rigid_mul(I,x):
    A6,mc,m=I[:,0:6],I[:,6:9],I[:,9]
    y=np.zeros((len(x),6),f)
    y[:,0]=A6[:,0]*x[:,0]+A6[:,1]*x[:,1]+A6[:,2]*x[:,2]
    y[:,1]=A6[:,1]*x[:,0]+A6[:,3]*x[:,1]+A6[:,4]*x[:,2]
    y[:,2]=A6[:,2]*x[:,0]+A6[:,4]*x[:,1]+A6[:,5]*x[:,2]
    y[:,0:3]+=cross(mc,x[:,3:6])
    t=cross(mc,x[:,0:3])
    y[:,3:6]=m[:,None]*x[:,3:6]-t
    return y
def crba32(blob,gc):
    N=len(gc); nb,nv=blob.nb,blob.nv
    q=gc.astype(f)
    ones=np.ones(N,f)
    R=[None]*nb; r=[None]*nb; S=[None]*nb
    w,x,y,z=q[:,3],q[:,4],q[:,5],q[:,6]
    inn=f(1)/np.sqrt(w*w+x*x+y*y+z*z); w,x,y,z=w*inn,x*inn,y*inn,z*inn
    two=f(2); one=f(1)
    R[0]=np.stack([one-two*(y*y+z*z),two*(x*y-w*z),two*(x*z+w*y),two*(x*y+w*z),one-two*(x*x+z*z),two*(y*z-w*x),two*(x*z-w*y),two*(y*z+w*x),one-two*(x*x+y*y)],1)
    r[0]=np.zeros((N,3),f); S[0]=np.zeros((N,6),f)
    for i in range(1,nb):
        p=blob.parent[i]
        ax=np.array(blob.axis[i][:],f); pt=np.tile(np.array(blob.ptree[i][:],f),(N,1)); rt=np.tile(np.array(blob.rtree[i][:],f),(N,1))
        qb=q[:,i+6]
        rev=blob.jtype[i]==1
        if rev:
            sn,cs=np.sin(qb),np.cos(qb); v=one-cs
            Rq=np.stack([cs+ax[0]*ax[0]*v, ax[0]*ax[1]*v-ax[2]*sn, ax[0]*ax[2]*v+ax[1]*sn,
                         ax[1]*ax[0]*v+ax[2]*sn, cs+ax[1]*ax[1]*v, ax[1]*ax[2]*v-ax[0]*sn,
                         ax[2]*ax[0]*v-ax[1]*sn, ax[2]*ax[1]*v+ax[0]*sn, cs+ax[2]*ax[2]*v],1).astype(f)
            E9=mm(rt,Rq)
        else: E9=rt
        R[i]=mm(R[p],E9)
        r[i]=r[p]+mv(R[p],pt)
        a3=mv(R[i],np.tile(ax,(N,1)))
        S[i]=np.zeros((N,6),f)
        if rev: S[i][:,0:3]=a3; S[i][:,3:6]=cross(r[i],a3)
        else: r[i]=r[i]+a3*qb[:,None]; S[i][:,3:6]=a3
    I10=[None]*nb
    for i in range(nb):
        cl=np.tile(np.array(blob.com[i][:],f),(N,1)); mass=f(blob.mass[i])
        c=r[i]+mv(R[i],cl)
        inn=np.array(blob.inertia[i][:],f)
        Il=np.tile(np.array([inn[0],inn[1],inn[2],inn[1],inn[3],inn[4],inn[2],inn[4],inn[5]],f),(N,1))
        Ri=R[i]; Tm=mm(Ri,Il)
        Iw=[Tm[:,0]*Ri[:,0]+Tm[:,1]*Ri[:,1]+Tm[:,2]*Ri[:,2], Tm[:,0]*Ri[:,3]+Tm[:,1]*Ri[:,4]+Tm[:,2]*Ri[:,5], Tm[:,0]*Ri[:,6]+Tm[:,1]*Ri[:,7]+Tm[:,2]*Ri[:,8],
            Tm[:,3]*Ri[:,3]+Tm[:,4]*Ri[:,4]+Tm[:,5]*Ri[:,5], Tm[:,3]*Ri[:,6]+Tm[:,4]*Ri[:,7]+Tm[:,5]*Ri[:,8], Tm[:,6]*Ri[:,6]+Tm[:,7]*Ri[:,7]+Tm[:,8]*Ri[:,8]]
        cc=c[:,0]*c[:,0]+c[:,1]*c[:,1]+c[:,2]*c[:,2]
        I=np.zeros((N,10),f)
        I[:,0]=Iw[0]+mass*(cc-c[:,0]*c[:,0]); I[:,1]=Iw[1]-mass*c[:,0]*c[:,1]; I[:,2]=Iw[2]-mass*c[:,0]*c[:,2]
        I[:,3]=Iw[3]+mass*(cc-c[:,1]*c[:,1]); I[:,4]=Iw[4]-mass*c[:,1]*c[:,2]; I[:,5]=Iw[5]+mass*(cc-c[:,2]*c[:,2])
        I[:,6]=mass*c[:,0]; I[:,7]=mass*c[:,1]; I[:,8]=mass*c[:,2]; I[:,9]=mass
        I10[i]=I
    for i in range(nb-1,0,-1): I10[blob.parent[i]]=I10[blob.parent[i]]+I10[i]
    M=np.zeros((N,nv,nv),f)
    I=I10[0]
    for k in range(3): M[:,k,k]=I[:,9]
    Bt=[0*I[:,0],I[:,8],-I[:,7],-I[:,8],0*I[:,0],I[:,6],I[:,7],-I[:,6],0*I[:,0]]
    for rr in range(3):
        for c2 in range(3): M[:,rr,3+c2]=Bt[3*rr+c2]; M[:,3+c2,rr]=Bt[3*rr+c2]
    M[:,3,3]=I[:,0];M[:,3,4]=I[:,1];M[:,3,5]=I[:,2];M[:,4,3]=I[:,1];M[:,4,4]=I[:,3];M[:,4,5]=I[:,4];M[:,5,3]=I[:,2];M[:,5,4]=I[:,4];M[:,5,5]=I[:,5]
    for i in range(1,nb):
        Fc=rigid_mul(I10[i],S[i]); di=i+5
        M[:,di,di]=dot6(S[i],Fc)+f(blob.armature[i])
        j=blob.parent[i]
        while j>=1:
            v=dot6(S[j],Fc); M[:,di,j+5]=v; M[:,j+5,di]=v; j=blob.parent[j]
        for k in range(3):
            M[:,di,k]=Fc[:,3+k];M[:,k,di]=Fc[:,3+k];M[:,di,3+k]=Fc[:,k];M[:,3+k,di]=Fc[:,k]
    assert M.dtype==f
    return M
def kernel_restated(Ms):
    A=Ms.copy(); N_,n,_=A.shape
    for j in range(n):
        d=A[:,j,j].copy()
        for k in range(j): d=d-A[:,j,k]*A[:,j,k]
        d=np.sqrt(d); A[:,j,j]=d; idd=f(1)/d
        for i in range(j+1,n):
            s=A[:,i,j].copy()
            for k in range(j): s=s-A[:,i,k]*A[:,j,k]
            A[:,i,j]=s*idd
    for i in range(n):
        ii=f(1)/A[:,i,i]
        for j in range(i):
            s=np.zeros(N_,f)
            for k in range(j,i): s=s+A[:,i,k]*(A[:,j,j] if k==j else A[:,k,j])
            A[:,i,j]=-s*ii
        A[:,i,i]=ii
    O=np.zeros_like(A)
    for a in range(n):
        for b in range(a+1):
            s=np.zeros(N_,f)
            for k in range(a,n): s=s+A[:,k,a]*A[:,k,b]
            O[:,a,b]=s;O[:,b,a]=s
    return O
if __name__=="__main__":
    for k in T.CASES:
        c=T.case(*k); j0=c.j0
        M32=crba32(c.model.blob,c.gc)
        Mr=c.M[:,j0:,j0:]
        eM=(np.abs(M32[:,j0:,j0:]-Mr).max(axis=(1,2))/np.abs(Mr).max(axis=(1,2))).max()
        Mi=kernel_restated(M32[:,j0:,j0:].copy()).astype(np.float64)
        res=np.abs(Mi@Mr-np.eye(Mr.shape[1])).max(axis=(1,2))
        conds=np.array([np.linalg.cond(m) for m in Mr])
        print(k,'nv',c.model.nv,'M rel err %.3g'%eM,'res max %.3g'%res.max(),'C max %.4g'%(res/(conds*T.EPS)).max())
